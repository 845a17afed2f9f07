"""Device engine: owns the HBM-resident matrices and drives the HIP kernels through the C-ABI.

Data layout in HBM (per GPU)
  X   : the U x I interaction matrix, replicated on every GPU, in BOTH orientations
        (CSC for the coordinate-descent column sweeps, CSR for X^T y and for scoring);
        int32 indices, float32 values -- 16 B per interaction in total.
  W   : this GPU's column shard [col_lo, col_hi) of the I x I item-item matrix, in the
        column-tiled CSR layout described in include/rtrec_amd.h (6 B per stored weight).
Nothing here computes on the host: numpy is used only to marshal index arrays.

Multi-GPU (one process per GPU, torch.distributed / RCCL): fit has no collective (each rank
fits the target columns it owns), scoring ends with one all-gather of the per-shard top-k
followed by the merge kernel.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp

from . import _native
from . import settings
# (round 4: the layout builders and the backend live in modules of their own; the names stay importable from here)
from .backend import DeviceWeights, HipBackend, XTY_SCRATCH_MAX_BYTES  # noqa: F401
from . import fit_plan, score_plan
# (the fit's constants live with the decision that uses them, in fit_plan.py; the names stay importable from here)
from .fit_plan import (FitFacts, FitKnobs, MAX_SLOTS, ALLF_OUTPUT_CAP, GRAM_ITEMS, GRAM_ITEMS_MAX, FIT_SCRATCH_GIB,  # noqa: F401
                       XTY_MIN_WALK_ENTRIES, FIT_HEAVY_TARGETS, FIT_HEAVY_SLOTS, FIT_HEAVY_MIN_ROWS, FIT_MW_MAX_TARGETS,
                       FIT_SLOTS_SPARSE, FIT_SPARSE_FEATURES, FIT_DENSE_FEATURES)
from .layouts import (TiledW, build_tiled_w, row_header_table, build_feature_rows, build_feature_rows_device,  # noqa: F401
                      build_tiled_w_device, _heavy_tiles_first, _pack_fragments, FR_MAX_ROWS, FR_MIN_FILL,
                      FR_TILE_HEADER_BYTES, FR_STREAM_BUF_BYTES)

DEFAULT_TILE_COLS = 4096   # 16 KB of float accumulators: 8 persistent waves per CU (2 per SIMD) hide each other's latency
DENSE_ROW_FILL = 1.0 / 3.0   # W row segments at least this full are stored dense (sparse layout)
GATHER_CHUNK_ROWS = 131072  # rows per exchange chunk of a column-sharded scoring call: a launch of the score kernel needs this
                            # many users to fill the chip a few times over (32k-row chunks: 6.4 ms per ML-20M pass against 2.6)
MAX_GATHER_CHUNKS = 8
ROW_CHUNK_ROWS = 49152     # least slots per exchange chunk of a row-sharded scoring call (each rank's launch per chunk): C4 at 8
                           # ranks (125k slots per rank) runs as two chunks, the gather of the first beside the kernel of the second


def sklearn_seed(random_state: Optional[int]) -> int:
    """The xorshift seed sklearn draws per ElasticNet.fit: check_random_state(rs).randint(0, 2**31-1)
    (sklearn/linear_model/_cd_fast.pyx:367).  random_state=43 -> 494155588."""
    return int(np.random.RandomState(random_state).randint(0, 2147483647))


def shard_bounds(n_items: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Item-column shard [lo, hi) owned by `rank` (contiguous blocks of ceil(I / G) columns)."""
    per = -(-n_items // world_size) if n_items > 0 else 0
    lo = min(n_items, rank * per)
    hi = min(n_items, lo + per)
    return lo, hi


def exchange_record_layout(k: int, f64: bool) -> Dict[str, int]:
    """The two per-user records of a column-sharded scoring call (_score_column_sharded), as offsets and widths in int32 words;
    a record is padded to an even number of them, so that consecutive records keep a leading float64 block 8-byte aligned:
    exchanged: [2k words of float64 scores]? | k scores | k ids | k aux | count | pad  (o_sc, o_ids, o_aux, o_cnt, width);
    final:     k scores | k ids | count | pad                                          (f_ids, f_cnt, fwidth)."""
    o_sc = 2 * k if f64 else 0
    o_ids, o_aux, o_cnt = o_sc + k, o_sc + 2 * k, o_sc + 3 * k
    f_ids, f_cnt = k, 2 * k
    width, fwidth = (n + 1 + ((n + 1) & 1) for n in (o_cnt, f_cnt))
    return {"o_sc": o_sc, "o_ids": o_ids, "o_aux": o_aux, "o_cnt": o_cnt, "width": width,
            "f_ids": f_ids, "f_cnt": f_cnt, "fwidth": fwidth}


def exchange_record_views(torch, recv, G: int, q: int, k: int, f64: bool):
    """The five arguments of `merge_topk` as views of a received [G * q, width] int32 record buffer (exchange_record_layout),
    [source shard, row, entry] each: (ids, float32 scores, float64 scores or None, aux, counts)."""
    L = exchange_record_layout(k, f64)
    g3 = recv.view(G, q, L["width"])
    g_sc64 = recv.view(torch.float64).view(G, q, L["width"] // 2)[:, :, :k] if f64 else None
    return (g3[:, :, L["o_ids"]:L["o_aux"]], g3[:, :, L["o_sc"]:L["o_ids"]].view(torch.float32), g_sc64,
            g3[:, :, L["o_aux"]:L["o_cnt"]], g3[:, :, L["o_cnt"]])


def spread_giant_rows(torch, order, lens, max_giants: int, giant_len: int):
    """The pattern-grouped work order with its giant rows spread out (SlimEngine._row_order).  A wave of the feature-row kernel
    takes CONSECUTIVE positions of that order (2, 4 or 8) and sets its users up one after the other; the few giant rows (tens of
    thousands of entries: they rate every feature item, so their patterns are neighbours at the head) must not share a wave --
    four of them in one wave made one of eight C4 row shards 0.81 ms instead of 0.59 (tools/row_slice_probe.py).  Up to
    `max_giants` rows of more than `giant_len` entries (`lens`: entries per row, indexed like the values of `order`) go to
    positions 0, 8, 16, ... of the head, longest first; the gaps are filled from the tail of the order (its lightest patterns);
    everything else keeps its place.  Returns a permutation of the same rows."""
    n_rows = int(order.numel())
    n_g = min(int(max_giants), n_rows // 64)
    if n_g <= 0:
        return order
    g_len, g_idx = torch.topk(lens, n_g)
    g_idx = g_idx[g_len > giant_len]
    n_g = int(g_idx.numel())
    if n_g == 0:
        return order
    is_g = torch.zeros(n_rows, dtype=torch.bool, device=order.device)
    is_g[g_idx] = True
    rest = order[~is_g[order]]
    n_fill = 7 * n_g
    head = torch.empty(8 * n_g, dtype=order.dtype, device=order.device)
    gap = torch.ones(8 * n_g, dtype=torch.bool, device=order.device)
    gap[0::8] = False
    head[0::8] = g_idx.to(order.dtype)
    head[gap] = rest[rest.numel() - n_fill:]
    return torch.cat([head, rest[:rest.numel() - n_fill]])


class SlimEngine:
    """Fit / score / similar-items on one GPU (one shard of W)."""

    _process_warm: set = set()          # devices whose code objects this process has loaded (see _process_warm_up)

    def __init__(self, device: Any = None, rank: int = 0, world_size: int = 1, process_group: Any = None,
                 tile_cols: Optional[int] = None, backend: Any = None, score_shard: Optional[str] = None,
                 warm_up: bool = True, shard_w: Optional[bool] = None):
        self.rank, self.world_size, self.group = rank, world_size, process_group
        # How a multi-GPU scoring pass is divided.  "columns" (default; BASELINE.json's configuration): every
        # rank scores all users against its item-column shard of W, lists are exchanged and merged.
        # "rows": W is replicated (it is assembled on every rank after a fit anyway), every rank scores its
        # 1/G slice of the users against all of W and only the final lists are all-gathered -- for
        # catalogues whose W is so small that a pass is bound by reading the user rows (C4: 3.2k active
        # columns), which column sharding does not divide.
        self.score_shard = (score_shard or settings.raw("RTREC_AMD_SCORE_SHARD", "columns")).lower()
        if self.score_shard not in ("columns", "rows"):
            raise ValueError(f"score_shard must be 'columns' or 'rows': {self.score_shard}")
        # shard_w (round 4; BASELINE.json: "W shards by item column across the 8 GPUs"): every rank FITS the item columns of its
        # own scoring shard [lo, hi) and keeps only those -- the fit output is the score input and W never moves.
        # Without it (the default) the targets are dealt out by column length and the coefficient triples are all-gathered, so
        # that every rank holds all of W: right while W is a few MB, not a design for a W that is not degenerate (500k
        # items x K=50 = 200 MB per copy and 8x the merge work).  Column-sharded scoring only; `item_similarity`,
        # `similar_items` and pickling gather on demand (collective calls: every rank must make them).
        if shard_w is None:
            shard_w = settings.raw("RTREC_AMD_SHARD_W", "0") == "1"
        self.shard_w = bool(shard_w) and world_size > 1 and self.score_shard == "columns"
        # testing aid: run the multi-GPU exchange (collectives, strided merge) even with a single rank, so that
        # the RCCL code path can be exercised on a one-GPU box through a 1-rank process group
        self.force_exchange = settings.raw("RTREC_AMD_FORCE_EXCHANGE") == "1"
        self.tile_cols = int(tile_cols or DEFAULT_TILE_COLS)
        self.be = backend if backend is not None else HipBackend(device)
        self._up = getattr(self.be, "to_dev_small", self.be.to_dev)      # host -> device for request-sized arrays
        self.n_users = 0
        self.n_items = 0
        self._X: Dict[str, Any] = {}
        self._W: Dict[str, Any] = {}
        self._F: Dict[str, Any] = {}       # resident factor vectors (set_factors)
        self._fit_ws: Dict[Tuple[int, int, int, int], Any] = {}
        self._score_ws = None
        self.gather_chunk_rows = GATHER_CHUNK_ROWS
        self.row_chunk_rows = ROW_CHUNK_ROWS
        self.last_fit_stats: Dict[str, Any] = {}
        self.score_timer = 0          # rtrec_timer handle (HipBackend.timer_create) bracketing the dominant score kernel
        self.use_feature_rows = settings.raw("RTREC_AMD_FEATURE_ROWS", "1") != "0"     # A/B switch of the score kernel
        # ablation switches of tools/score_ablate.sh: only a diagnostic build of the library looks at them
        self.diagnostics = int(settings.raw("RTREC_AMD_ABLATE", "0")) & 0xff
        self.fr_users_per_wave = int(settings.raw("RTREC_AMD_FR_USERS", "0"))      # 8 / 4 / 2: force the feature-row kernel's form
        self.fr_head_kib = int(settings.raw("RTREC_AMD_FR_HEAD_KIB", "-1"))        # 0 .. 126: cap of the feature-row kernel's resident head
        self.native_seg_builder = settings.raw("RTREC_AMD_NATIVE_SEG_BUILD", "1") != "0"   # csrc/seg_build.hip (else tensor ops)
        self.FR_SMALL_BATCH = int(settings.raw("RTREC_AMD_FR_SMALL_BATCH", self.FR_SMALL_BATCH))     # A/B: segments for larger passes
        self.f64_refine = settings.raw("RTREC_AMD_F64_REFINE", "1") != "0"      # float64 W: float32 fast pass + float64 refine
        self.cands_direct = settings.raw("RTREC_AMD_CANDS_DIRECT", "1") != "0"   # request-sized CANDIDATES calls: csrc/score_cands.hip
        self.dense_fast = settings.raw("RTREC_AMD_DENSE_FAST", "1") != "0"    # DENSE mode through the fast SPARSE-style pass
        self.dense_fill = settings.raw("RTREC_AMD_DENSE_FILL", "1") != "0"    # ... its short lists completed in place (and so column shards)
        self._sg_scratch = None           # zeroed scratch of the segment path's workgroup-per-user kernel
        self._order_grouped = False       # the work order _row_order handed out last is the pattern-grouped one
        self.sg_heavy_min = int(settings.raw("RTREC_AMD_SG_HEAVY_MIN", "0"))   # v > 0: segment path, users of more than v - 1 items get a workgroup
        self.use_seg_layout = settings.raw("RTREC_AMD_SEG_LAYOUT", "1") != "0"        # A/B switch of the general-W score kernel
        self.seg_cluster = settings.raw("RTREC_AMD_SEG_CLUSTER", "1") != "0"          # ... and of its column clustering
        self.use_seg_heavy = settings.raw("RTREC_AMD_SEG_HEAVY", "1") != "0"          # ... and of its workgroup-per-long-user pass
        self.lazy_tiled = settings.raw("RTREC_AMD_LAZY_TILED", "1") != "0"           # tiled layout only when a call flags exact ties
        self.last_score_path = ""     # which kernel family served the last _local_topk call (tests, bench.py)
        self._sg_labels = None        # (cluster labels of the last segment layout, n_items, nnz of W when they were computed)
        if warm_up and isinstance(self.be, HipBackend) and str(self.be.device) not in SlimEngine._process_warm:
            SlimEngine._process_warm.add(str(self.be.device))
            self._process_warm_up()

    def _process_warm_up(self) -> None:
        """Once per process and device: a toy model through the whole path (fit, write-back, every layout builder, every
        scoring mode) on a throw-away engine.  The first use of a kernel -- ours or one of the tensor ops of the builders --
        loads its code object (tens of milliseconds each: the first W write-back of a process took 120-320 ms, the first
        layouts 60-90 ms); that belongs next to the creation of the HIP context, not inside the first fit or recommend."""
        rng = np.random.default_rng(0)
        U, I = 96, 48
        X = sp.random(U, I, density=0.3, random_state=rng, format="csr", dtype=np.float32)
        X.data[:] = rng.integers(1, 6, X.nnz).astype(np.float32)
        Xc = X.tocsc()
        Xc.sort_indices()
        X.sort_indices()
        toy = SlimEngine(backend=self.be, rank=0, world_size=1, warm_up=False)
        try:
            toy.set_interactions(Xc, X)
            for mode in ("exact", "gram"):
                out = toy.fit_columns(np.arange(I), nn_feature_selection=8, device_out=True, mode=mode)
            dw = toy.merge_fit(None, I, False, *out[:4])
            dw = toy.merge_fit(dw, I, False, *out[:4])                      # the merge into an existing W as well
            rows = np.arange(U)
            for f64 in (False, True):
                toy.set_weights(dw, acc_f64=f64)
                for md in (_native.TOPK_SPARSE, _native.TOPK_DENSE):
                    toy.recommend_rows(rows, top_k=5, mode=md)              # fast layouts, flagged rows -> tiled layouts
                    toy.recommend_rows(rows[:3], top_k=5, mode=md)          # the request-sized path
            toy.set_weights(dw, acc_f64=False)
            toy._layout(True, 5)
            toy._layout(False, 5)
            # the tensor ops of the write-back and the builders pick other kernel configurations for real sizes (radix sort,
            # scans, compaction): once more on a quarter of a million elements
            torch = self.be.torch
            big = torch.arange(1 << 18, dtype=torch.int64, device=self.be.device).flip(0)
            srt, order = torch.sort(big)
            _ = (torch.argsort(big), torch.unique(big % 1000), big[big % 2 == 0], torch.isin(big, big[:100]), torch.cumsum(big, 0),
                 torch.searchsorted(srt, big[:1000]), torch.nonzero(big % 3 == 0), torch.repeat_interleave(big[:1000] % 7),
                 torch.bincount(big % 1000), big.to(torch.int32).to(torch.float32).abs().max(), torch.cat([big, big]),
                 torch.sort(big.to(torch.float32), descending=True), torch.argsort(big % 977, stable=True))
            self.be.synchronize()
        except Exception as e:          # a warm-up must never keep an engine from being constructed -- but it must not hide a
            # broken library either: say so, and surface / clear pending device errors now
            logging.warning(f"rtrec_amd warm-up failed (the first real call will hit the same problem): {e!r}")
            try:
                self.be.synchronize()
            except Exception as e2:
                logging.warning(f"rtrec_amd: device error after the failed warm-up: {e2!r}")

    # ------------------------------------------------------------------------------ X
    def set_interactions(self, X_csc: sp.csc_matrix, X_csr: Optional[sp.csr_matrix] = None,
                         need_csc: bool = True) -> None:
        """Upload X (U x I).  Both orientations must have sorted indices (scipy canonical form)."""
        be = self.be
        if X_csr is None and need_csc and getattr(be, "supports_device_store", False):
            # only the CSC orientation comes from the host: the CSR one is a sort of the keys on the device
            # (utils/device_store.py) instead of a scipy tocsr() here and a second upload
            from .utils.device_store import DeviceInteractions
            if not X_csc.has_sorted_indices:
                X_csc = X_csc.sorted_indices()
            if X_csc.nnz >= 2 ** 31:
                raise ValueError("more than 2**31 interactions per GPU are not supported")
            d = DeviceInteractions(be.torch, be.device)
            d.load_csc(X_csc.indptr, X_csc.indices, X_csc.data, X_csc.shape[0], X_csc.shape[1], 0)
            self.set_interactions_device(d.full(), X_csc.shape[0], X_csc.shape[1])
            return
        if X_csr is None:
            X_csr = X_csc.tocsr()
        if not X_csr.has_sorted_indices:
            X_csr = X_csr.sorted_indices()
        self.n_users, self.n_items = X_csr.shape
        if X_csr.nnz >= 2 ** 31:
            raise ValueError("more than 2**31 interactions per GPU are not supported")
        X: Dict[str, Any] = {}
        X["rptr"] = be.to_dev(np.asarray(X_csr.indptr, dtype=np.int32))
        X["rcol"] = be.to_dev(np.asarray(X_csr.indices, dtype=np.int32))
        X["rval"] = be.to_dev(np.asarray(X_csr.data, dtype=np.float32))
        if need_csc:
            if X_csc is None:
                X_csc = X_csr.tocsc()
            if not X_csc.has_sorted_indices:
                X_csc = X_csc.sorted_indices()
            X["cptr"] = be.to_dev(np.asarray(X_csc.indptr, dtype=np.int32))
            X["crow"] = be.to_dev(np.asarray(X_csc.indices, dtype=np.int32))
            X["cval"] = be.to_dev(np.asarray(X_csc.data, dtype=np.float32))
            X["col_nnz"] = np.diff(np.asarray(X_csc.indptr, dtype=np.int64))
            X["nonneg"] = bool(X_csc.nnz == 0 or float(X_csc.data.min()) >= 0.0)
        self._X = X

    def set_interactions_device(self, X: Dict[str, Any], n_users: int, n_items: int) -> None:
        """Use an X whose arrays are already resident on this device (utils/device_store.py): the same
        keys as set_interactions builds (rptr/rcol/rval, cptr/crow/cval, col_nnz, nonneg)."""
        if int(X["rcol"].shape[0]) >= 2 ** 31:
            raise ValueError("more than 2**31 interactions per GPU are not supported")
        self.n_users, self.n_items = int(n_users), int(n_items)
        self._X = dict(X)          # per-matrix caches (column norms, Gram matrix) attach to this copy

    # ------------------------------------------------------------------------------ fit
    def owned_columns(self, columns: np.ndarray) -> np.ndarray:
        """The part of `columns` (the same list on every rank) THIS rank fits.  Fitting has no
        collective and a popular item costs far more than a rare one, so the targets are dealt out
        by column length: sorted by nnz(X[:, j]) descending and dealt in snake order (ranks 0..G-1,
        then G-1..0, ...) -- every rank gets the same mix of heavy and light targets.  Which
        rank fitted a column is independent of which rank scores it: W is assembled on every rank
        after the fit and re-sharded by contiguous column block for scoring (shard_bounds)."""
        columns = np.asarray(columns, dtype=np.int64)
        if self.world_size == 1:
            return columns
        if self.shard_w:        # the rank that scores a column fits it: W never moves
            lo, hi = shard_bounds(self.n_items, self.world_size, self.rank)
            return np.sort(columns[(columns >= lo) & (columns < hi)])
        nnz = self._X["col_nnz"][columns] if "col_nnz" in self._X else np.zeros(len(columns), dtype=np.int64)
        order = np.lexsort((columns, -nnz))            # nnz descending, ties by id: identical on all ranks
        pos = np.arange(len(columns))
        blk, off = pos // self.world_size, pos % self.world_size
        owner = np.where(blk % 2 == 0, off, self.world_size - 1 - off)
        return np.sort(columns[order[owner == self.rank]])

    def fit_columns(self, targets: Sequence[int], alpha: float = 0.1, l1_ratio: float = 0.1,
                    positive: bool = True, max_iter: int = 100, tol: float = 1e-4, random_state: Optional[int] = 43,
                    nn_feature_selection: Optional[int] = None, n_slots: Optional[int] = None,
                    trace: bool = False, exact: bool = True, mode: Optional[str] = None, device_out: bool = False
                    ) -> Tuple[Any, Any, Any, Any, np.ndarray]:
        """Fit the given target columns on this GPU.  mode: "exact" (default; bit-identical to scikit-learn),
        "gram" (Gram-form coordinate descent where all features are in the Gram matrix, tree-reduced dots elsewhere;
        a few 1e-5 relative; what exact=False selects) or "shuffle" (tree-reduced dots only) -- rtrec_fit_opts.fast.

        Returns (targets_in_processing_order, items[n, cap], coef[n, cap], count[n], n_iter[n]);
        row t describes model.sparse_coef_ of target t (see rtrec_slim_fit_columns).  device_out=True (feature
        selection only) leaves the first four on the device -- int32 targets, the kernels' output blocks -- for
        merge_fit(); only n_iter (one int per target) is downloaded.

        What the call asks of the device is decided by fit_plan.plan_fit; this method runs that plan.
        """
        be, X = self.be, self._X
        if "cptr" not in X:
            raise RuntimeError("set_interactions() with the CSC orientation must be called before fit_columns()")
        U, I = self.n_users, self.n_items
        targets = np.asarray(targets, dtype=np.int64)
        distinct_targets = len(np.unique(targets)) == len(targets)
        # longest columns first: the device work queue then ends on short jobs
        targets = targets[np.argsort(-X["col_nnz"][targets], kind="stable")]
        K = int(nn_feature_selection) if nn_feature_selection is not None else 0
        if nn_feature_selection is not None and K <= 0:
            raise AssertionError(f"n_neighbors must be a positive integer: {K}")
        cfg = _native.FitCfg(np.float32(alpha * l1_ratio * U), np.float32(alpha * (1.0 - l1_ratio) * U),
                             np.float32(tol), int(max_iter), sklearn_seed(random_state), int(bool(positive)), K)
        torch = be.torch
        if "sqn" not in X:
            X["sqn"] = be.empty((I,), torch.float32)
            be.column_sqnorms(I, X["cptr"], X["cval"], X["sqn"])
        n = len(targets)
        knobs = FitKnobs.from_settings()
        plan = fit_plan.plan_fit(FitFacts(
            n_users=U, n_items=I, n_targets=n, col_nnz=X["col_nnz"][targets], nnz=int(X["col_nnz"].sum()), K=K,
            mode=mode or ("exact" if exact else "gram"), n_slots=n_slots, device_out=device_out, nonneg=bool(X.get("nonneg")),
            hip=isinstance(be, HipBackend), supports_gram=getattr(be, "supports_gram", False), distinct_targets=distinct_targets,
            pilot_density=lambda: self._pilot_feature_density(targets, cfg, knobs)), knobs)
        cap = plan.cap
        gram = None
        if plan.use_gram:
            n_top = self._gram_items(targets, cfg, knobs)
            if X.get("gram_n") != n_top:
                X["gram"], X["gram_n"] = be.gram_matrix(X, U, I, n_top), n_top
            gram = X["gram"]

        # device_out keeps the launches' blocks (`kept`), otherwise each is downloaded into `host` before the next launch
        kept: List[Tuple[int, Dict[str, Any]]] = []
        host = None if device_out else dict(items=np.empty((n, cap), dtype=np.int32), coef=np.empty((n, cap), dtype=np.float32),
                                            count=np.empty((n,), dtype=np.int32), niter=np.empty((n,), dtype=np.int32))
        trace_out = np.zeros((n, 8), dtype=np.int64) if trace else None
        heavy = side = None
        for ln in plan.launches:
            args = (targets[ln.lo:ln.hi], cfg, cap, ln.n_slots, ln.role, knobs, plan.slots, trace, gram, plan.fast, ln.one_pass_xty)
            if ln.role == "heavy":      # on the side stream, beside the chunks; collected after them
                side = self._side_stream = getattr(self, "_side_stream", None) or torch.cuda.Stream(be.device)
                side.wait_stream(torch.cuda.current_stream(be.device))
                with torch.cuda.stream(side):
                    heavy = (ln, self._launch_fit(*args))
            else:
                self._collect_fit(ln, self._launch_fit(*args), host, kept, trace_out)
        if heavy is not None:
            torch.cuda.current_stream(be.device).wait_stream(side)
            self._collect_fit(*heavy, host, kept, trace_out)
        if K <= 0 and cap < I:
            over = np.flatnonzero(host["count"] > cap)
            if over.size:      # K = None targets whose solution did not fit the output block: refit these with room for every item, then widen the block
                d = self._launch_fit(targets[over], cfg, I, max(1, min(plan.slots, len(over))), "overflow", knobs)
                full = {k: d[k].cpu().numpy() for k in ("items", "coef", "count", "niter")}
                wide = int(max(int(full["count"].max()), cap))
                items_w = np.zeros((n, wide), dtype=np.int32); items_w[:, :cap] = host["items"]
                coef_w = np.zeros((n, wide), dtype=np.float32); coef_w[:, :cap] = host["coef"]
                items_w[over] = full["items"][:, :wide]; coef_w[over] = full["coef"][:, :wide]
                host["niter"][over] = full["niter"]
                host["items"], host["coef"] = items_w, coef_w
        self.last_fit_stats = {"n_targets": n, "slots": plan.slots, "cap": cap, "trace": trace_out, "n_heavy": plan.n_heavy,
                               "plan": plan}
        self.last_fit_targets = targets
        if device_out:
            kept.sort(key=lambda e: e[0])
            cat = (lambda k, shape, dt: torch.cat([d[k] for _, d in kept]) if kept else be.empty(shape, dt))
            d_niter = cat("niter", (0,), torch.int32)
            return (cat("t", (0,), torch.int32), cat("items", (0, cap), torch.int32), cat("coef", (0, cap), torch.float32),
                    cat("count", (0,), torch.int32), d_niter.cpu().numpy())
        return targets, host["items"], host["coef"], host["count"], host["niter"]

    def _fit_workspace(self, n_slots: int, K: int, role: str = "main", limit: int = 0):
        """(scratch, queue, slots of the scratch layout) -- the one scratch cache of the fit.  `role` keeps the side-stream
        launch of the heavy targets on a scratch of its own (the two kernels run concurrently).  main / heavy: a cached scratch
        of the same problem shape with at least n_slots slots is reused as it is -- the kernel launches min(slots, targets)
        workgroups, so extra slots are simply idle -- which keeps mini-batches of varying size (online partial_fit) from
        re-allocating and re-initialising it every call; a new one is rounded up to a power of two, but not beyond `limit`
        (the call's slots in flight).  The overflow refit's is sized exactly; the pilot's too, and is not kept."""
        be, U, I = self.be, self.n_users, self.n_items
        if role == "pilot":
            return (*be.fit_workspace(U, I, n_slots, K), n_slots)
        if role == "overflow":
            key = (U, I, n_slots, K, role)
            if key not in self._fit_ws:
                self._fit_ws[key] = be.fit_workspace(U, I, n_slots, K)
        else:
            fits = [k for k in self._fit_ws if k[0] == U and k[1] == I and k[3] == K and k[2] >= n_slots and k[4] == role]
            if fits:
                key = min(fits, key=lambda k: k[2])
            else:
                want = 1 << max(0, int(n_slots - 1).bit_length())          # next power of two
                key = (U, I, int(min(max(want, n_slots), max(limit, n_slots))), K, role)
                if len(self._fit_ws) >= 4:
                    self._fit_ws.clear()
                self._fit_ws[key] = be.fit_workspace(U, I, key[2], K)
        ws, queue = self._fit_ws[key]
        return ws, queue, key[2]

    def _launch_fit(self, tg: np.ndarray, cfg, cap: int, n_slots: int, role: str, knobs: FitKnobs, limit: int = 0,
                    trace: bool = False, gram=None, fast: int = 0, one_pass_xty: bool = False) -> Dict[str, Any]:
        """The only caller of be.fit_columns: allocates the output block of targets `tg`, fetches the scratch of `role`
        and launches on the current stream.  A new kernel option is an argument here and nowhere else.  Returns the device block."""
        be, torch = self.be, self.be.torch
        m = len(tg)
        ws, queue, ws_slots = self._fit_workspace(n_slots, int(cfg.top_features), role, limit)
        d = dict(t=be.to_dev(tg.astype(np.int32)), items=be.empty((m, cap), torch.int32),
                 coef=be.empty((m, cap), torch.float32), count=be.empty((m,), torch.int32),
                 niter=be.empty((m,), torch.int32), trace=be.zeros((m, 8), torch.int64) if trace else None,
                 ws=(ws, queue))   # keeps the scratch alive while the kernel runs
        # how the HIP kernels are to go about it; the tests' CPU stand-in solves target by target and takes none of these
        opts = dict(fast=fast, one_pass_xty=one_pass_xty, knobs=knobs) if getattr(be, "fit_launch_options", False) else {}
        be.fit_columns(self.n_users, self.n_items, self._X, d["t"], cfg, d["items"], d["coef"], d["count"], d["niter"], cap, ws, queue,
                       ws_slots, d["trace"], gram, **opts)
        return d

    @staticmethod
    def _collect_fit(ln, d: Dict[str, Any], host, kept, trace_out) -> None:
        if trace_out is not None:
            trace_out[ln.lo:ln.hi] = d["trace"].cpu().numpy()
        if host is None:
            kept.append((ln.lo, d))
            return
        for k in ("items", "coef", "count", "niter"):
            host[k][ln.lo:ln.hi] = d[k].cpu().numpy()

    SGD_EPOCH_BLOCK_BYTES = 2 << 30   # time-sorted copies of X held at once by fit_columns_sgd (8 B per stored entry and epoch)

    def fit_columns_sgd(self, targets: Sequence[int], alpha: float = 0.1, l1_ratio: float = 0.1, eta0: float = 0.001,
                        max_iter: int = 100, tol: Optional[float] = 1e-4, random_state: Optional[int] = 43,
                        nn_feature_selection: Optional[int] = None):
        """optim="sgd" (slim_elastic.py:209-222): scikit-learn's SGDRegressor behind FeatureSelectionWrapper, one model per
        target column, bit-identical coef_ and n_iter_ (csrc/fit_sgd.hip; oracle: slim_oracle_sgd).  Returns device tensors
        (targets, items [n, K] in selection order, coef [n, K], count [n]) and n_iter (numpy) like
        fit_columns(device_out=True).  Steps: (1) the X^T y / top-K selection of the coordinate-descent kernel (one sweep,
        coefficients dropped); (2) per block of epochs the host schedule (shuffled sample order, learning rates, weight
        scale, cumulative L1 penalty: target-independent) and one device sort of X's entries by (column, time); (3) the
        solver kernel, one wave per target, until every target has stopped (n_iter_no_change = 5) or max_iter is reached.
        The solver is strictly sequential in the samples: U x epochs dependent steps per target (the reference's cost too)."""
        if nn_feature_selection is None:
            # the reference itself fails here (slim_elastic.py:273: SGDRegressor has no sparse_coef_)
            raise AttributeError("'SGDRegressor' object has no attribute 'sparse_coef_'")
        be, X = self.be, self._X
        U, I = self.n_users, self.n_items
        K = min(int(nn_feature_selection), I)
        if K <= 0:
            raise AssertionError(f"n_neighbors must be a positive integer: {K}")
        targets = np.asarray(targets, dtype=np.int64)
        if not isinstance(be, HipBackend):
            return be.fit_columns_sgd(X, U, I, targets, alpha, l1_ratio, eta0, max_iter, tol, random_state, K)
        if K > self.SGD_MAX_FEATURES:
            raise NotImplementedError(f"optim='sgd' on the GPU serves nn_feature_selection <= {self.SGD_MAX_FEATURES} "
                                      "(up to four features per wave lane)")
        torch = be.torch
        # (1) feature selection: the coordinate-descent kernel's own X^T y + top-K (its item lists come in selection order)
        d_t, d_sel, _coef, d_cnt, _ = self.fit_columns(targets, alpha=alpha, l1_ratio=l1_ratio, positive=True, max_iter=1,
                                                      tol=1e-4, random_state=random_state, nn_feature_selection=K,
                                                      device_out=True, mode="exact")
        n = int(d_t.numel())
        cap = int(d_sel.shape[1]) if n else K
        if n == 0:
            return d_t, d_sel, be.empty((0, cap), torch.float32), d_cnt, np.empty(0, np.int32)
        d_sel, d_cnt = d_sel.contiguous(), d_cnt.contiguous()
        nnz = int(X["crow"].numel())
        tol_ = float("-inf") if tol is None else float(tol)
        seed = sklearn_seed(random_state)
        col_of = torch.repeat_interleave(torch.arange(I, device=X["crow"].device, dtype=torch.int64),
                                         (X["cptr"][1:] - X["cptr"][:-1]).long())
        crow64 = X["crow"].long()
        block = int(max(1, min(int(max_iter), self.SGD_EPOCH_BLOCK_BYTES // max(8 * nnz, 1), 16)))
        d_w, d_q = be.zeros((n, cap), torch.float32), be.zeros((n, cap), torch.float32)
        d_best = torch.full((n,), float("inf"), dtype=torch.float64, device=be.device)
        d_noimp, d_niter = be.zeros((n,), torch.int32), be.zeros((n,), torch.int32)
        d_unf = be.zeros((1,), torch.int32)
        order = np.arange(U, dtype=np.int32)
        state = np.array([1.0, 0.0, 1.0], dtype=np.float64)
        p, hp = be.ptr, (lambda a: C.c_void_p(a.ctypes.data))
        first = 0
        while first < max_iter:
            ne = min(block, max_iter - first)
            steps = ne * U
            time_of = np.empty((ne, U), dtype=np.int32)
            eta, wsb, wsa, ua = (np.empty(steps, dtype=np.float64) for _ in range(4))
            rcnt = np.empty(steps + 1, dtype=np.int32)
            rmult = np.empty(steps + 1, dtype=np.float32)
            n_res = C.c_int32(0)
            _native.check(be.lib.rtrec_slim_sgd_schedule(U, ne, seed, float(alpha), float(l1_ratio), float(eta0), 0.25, hp(order),
                                                         hp(state), hp(time_of), hp(eta), hp(wsb), hp(wsa), hp(ua), hp(rcnt),
                                                         hp(rmult), steps + 1, C.byref(n_res)), "rtrec_slim_sgd_schedule")
            d_time_of = be.to_dev(time_of)
            d_tt = be.empty((ne, nnz), torch.int32)
            d_tv = be.empty((ne, nnz), torch.float32)
            for e in range(ne):        # every column's entries by their time in this epoch (stable in the column: keys are distinct)
                key = col_of * U + d_time_of[e].long()[crow64]
                skey, perm = torch.sort(key)
                d_tt[e] = (skey % U).to(torch.int32)
                d_tv[e] = X["cval"][perm]
            d_eta, d_wsb, d_wsa, d_ua = (be.to_dev(a) for a in (eta, wsb, wsa, ua))
            d_rcnt, d_rmult = be.to_dev(rcnt), be.to_dev(rmult[:max(int(n_res.value), 1)].copy())
            be.ops.fit_sgd_epochs(X["cptr"], d_tt, d_tv, d_t, d_sel, d_cnt, U, I, nnz, cap, first, ne, int(max_iter), tol_, d_eta, d_wsb,
                                  d_wsa, d_ua, d_rcnt, d_rmult, d_w, d_q, d_best, d_noimp, d_niter, d_unf)
            first += ne
            if int(d_unf.item()) == 0:
                break
        n_iter = d_niter.cpu().numpy()
        if (n_iter < 0).any():
            # n_iter follows d_t, the order fit_columns processed the targets in (longest column first), not the caller's:
            # name the first column of the caller's list that failed, as a fit column by column would
            failed = set(d_t.cpu().numpy()[n_iter < 0].tolist())
            raise ValueError("Floating-point under-/overflow occurred during the SGD fit of column "
                             f"{next(int(j) for j in targets if int(j) in failed)}. Scaling input data with StandardScaler or "
                             "MinMaxScaler might help.")
        return d_t, d_sel, d_w, d_cnt, n_iter

    SGD_MAX_FEATURES = 256           # csrc/fit_sgd.hip: kSgdMaxFeatures

    GRAM_PILOT_TARGETS = fit_plan.GRAM_PILOT_TARGETS
    GRAM_PILOT_MIN_NNZ = fit_plan.GRAM_PILOT_MIN_NNZ      # (an attribute so that a test can reach the pilot on a small matrix)

    def _pilot_feature_density(self, targets: np.ndarray, cfg, knobs: FitKnobs) -> Optional[float]:
        """Mean density of the feature columns the Gram pilot selected (fit_plan.fit_slots_for_density); None: no pilot."""
        if "pilot_feature_density" not in self._X:
            self._gram_items(targets, cfg, knobs)            # runs the pilot when the call is large enough for one
        return self._X.get("pilot_feature_density")

    def _gram_items(self, targets: np.ndarray, cfg, knobs: FitKnobs) -> int:
        """How many of the most popular item columns the shared Gram matrix covers (RTREC_AMD_GRAM_ITEMS=<n> fixes it):
        fit_plan.gram_items, from a pilot where fit_plan.gram_pilot_pays.  The answer is cached with X."""
        X = self._X
        if knobs.gram_items is not None:
            return min(self.n_items, knobs.gram_items)
        if "gram_auto" not in X:
            col_nnz = X["col_nnz"]
            nonempty = int(np.count_nonzero(col_nnz))
            pilot = fit_plan.gram_pilot_pays(len(targets), isinstance(self.be, HipBackend), int(cfg.top_features), nonempty,
                                             int(col_nnz.sum()), self.GRAM_PILOT_MIN_NNZ)
            X["gram_auto"] = fit_plan.gram_items(self.n_items, nonempty, self._gram_pilot(targets, cfg, knobs) if pilot else None)
        return X["gram_auto"]

    def _gram_pilot(self, targets: np.ndarray, cfg, knobs: FitKnobs) -> Optional[int]:
        """The feature selection (one sweep) of 64 of the call's targets from the middle of the length-sorted list.  Returns
        the 90th percentile of the deepest popularity rank a target selects, plus one (None: no target has an entry), and
        leaves the mean density of the selected columns in X["pilot_feature_density"]."""
        X, col_nnz = self._X, self._X["col_nnz"]
        live = targets[col_nnz[targets] > 0]
        if not len(live):
            return None
        # (not the head of the length-sorted list: a popular target's X^T y walks 100k user rows, and what it selects is no
        # different -- the pilot costs a few ms this way instead of ~100)
        pick = live[np.linspace(0.05 * (len(live) - 1), 0.6 * (len(live) - 1), min(self.GRAM_PILOT_TARGETS, len(live))).astype(np.int64)]
        m = len(pick)
        pcfg = _native.FitCfg(cfg.l1_reg, cfg.l2_reg, cfg.tol, 1, cfg.seed, cfg.positive, cfg.top_features)
        d = self._launch_fit(pick, pcfg, min(int(cfg.top_features), self.n_items), m, "pilot", knobs)
        rank = np.empty(self.n_items, dtype=np.int64)
        rank[np.argsort(-col_nnz, kind="stable")] = np.arange(self.n_items)
        it, cn = d["items"].cpu().numpy(), d["count"].cpu().numpy()
        deepest = np.array([rank[it[k, :cn[k]]].max() if cn[k] else 0 for k in range(m)])
        sel = np.concatenate([it[k, :cn[k]] for k in range(m)]) if cn.sum() else np.empty(0, np.int64)
        if len(sel):          # how dense the columns a target folds are (fit_plan.fit_slots_for_density)
            X["pilot_feature_density"] = float(col_nnz[sel].mean()) / max(self.n_users, 1)
        return int(np.percentile(deepest, 90)) + 1

    # ------------------------------------------------------------------------------ W
    def upload_weights(self, W_csc: sp.csc_matrix, acc_f64: Optional[bool] = None) -> DeviceWeights:
        """Host W (I x I, CSC) -> DeviceWeights (weights are float32 on the device, like every layout built from them)."""
        be, torch = self.be, self.be.torch
        W_csc = W_csc if W_csc.has_sorted_indices else W_csc.sorted_indices()
        n_items = W_csc.shape[1]
        data = np.asarray(W_csc.data)
        nz = data != 0
        cols = np.repeat(np.arange(n_items, dtype=np.int64), np.diff(W_csc.indptr))
        f64 = bool(W_csc.dtype == np.float64) if acc_f64 is None else bool(acc_f64)
        d32 = data[nz].astype(np.float32)
        lossy = bool(data.dtype != np.float32 and not np.array_equal(d32.astype(data.dtype), data[nz]))
        return DeviceWeights(be.to_dev(np.asarray(W_csc.indices, dtype=np.int64)[nz]), be.to_dev(cols[nz]), be.to_dev(d32),
                             n_items, f64, host=W_csc if nz.all() else None, lossy=lossy)

    def set_weights(self, W: Any, acc_f64: Optional[bool] = None) -> None:
        """Register W: a host scipy CSC matrix (uploaded) or a DeviceWeights (what merge_fit returns: nothing moves).
        The layouts of this rank's column shard are built ON THE DEVICE on first use: a compacted one (columns with
        at least one weight) plus the feature-row form for SPARSE mode, a plain one for DENSE / CANDIDATES mode."""
        dw = W if isinstance(W, DeviceWeights) else self.upload_weights(W, acc_f64)
        if acc_f64 is not None:
            dw.f64 = bool(acc_f64)
        n_items = dw.n_items
        lo, hi = (0, n_items) if self.score_shard == "rows" else shard_bounds(n_items, self.world_size, self.rank)
        self._W = {"n_items": n_items, "col_lo": lo, "col_hi": hi, "acc_f64": dw.f64, "dw": dw, "layouts": {}}
        self._X.pop("_orders", None)           # work orders are per layout

    @property
    def weights(self) -> Optional[DeviceWeights]:
        return self._W.get("dw") if self._W else None

    def merge_fit(self, old: Optional[DeviceWeights], n_items: int, f64: bool, d_targets, d_items, d_coef, d_count
                  ) -> DeviceWeights:
        """The LIL write-back of slim_elastic.py:271-274 / 371-374 / 554-557 on the device: start from `old`, then for
        every fitted (i, j) a non-zero value overwrites W[i, j] and an explicit zero deletes it; entries of column j
        that the new solution does not mention survive.  The arguments are this rank's
        fit_columns(device_out=True) tensors; with several ranks the triples are exchanged on the device
        (_all_gather_triples) -- nothing is pickled and nothing visits the host."""
        torch = self.be.torch
        n, cap = d_items.shape
        mask = torch.arange(cap, device=d_items.device)[None, :] < d_count[:, None]
        key = (d_targets.to(torch.int64)[:, None] * n_items + d_items.to(torch.int64))[mask]
        val = d_coef[mask]
        if self.world_size > 1 and not self.shard_w:
            key, val = self._all_gather_triples(key, val)
        if self.shard_w and old is not None and (getattr(old, "shard", None) is None or old.n_items != n_items):
            # the catalogue grew (the block boundaries moved) or the old W was not sharded: every rank keeps the old entries
            # of ITS columns under the new boundaries
            old = self.gather_weights(old)
            lo, hi = shard_bounds(n_items, self.world_size, self.rank)
            sel = (old.cols >= lo) & (old.cols < hi)
            old = DeviceWeights(old.rows[sel], old.cols[sel], old.vals[sel], old.n_items, old.f64)
        if old is not None and old.nnz:
            inside = (old.rows < n_items) & (old.cols < n_items)
            o_key = (old.cols * n_items + old.rows)[inside]
            keep = ~torch.isin(o_key, key)
            key = torch.cat([o_key[keep], key])
            val = torch.cat([old.vals[inside][keep], val])
        nz = val != 0
        key, val = key[nz], val[nz]
        order = torch.argsort(key)
        key = key[order]
        dw = DeviceWeights(key % n_items, key // n_items, val[order].contiguous(), n_items, f64)
        if self.shard_w:
            dw.shard = (self.rank, self.world_size)
        return dw

    def _all_gather_triples(self, key, val):
        """Every rank's (int64 key, float32 value) triples, concatenated in rank order: all_gather_into_tensor of the parts,
        each padded to the longest one (only the part sizes visit the host).  A COLLECTIVE: every rank calls it."""
        import torch.distributed as dist
        torch, G, dev = self.be.torch, self.world_size, key.device
        sizes = torch.zeros(G, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(sizes, torch.tensor([key.numel()], dtype=torch.int64, device=dev), group=self.group)
        sizes = sizes.cpu().tolist()
        m = max(max(sizes), 1)
        out = []
        for part in (key, val):
            padded = torch.zeros(m, dtype=part.dtype, device=dev); padded[:part.numel()] = part
            every = torch.empty(m * G, dtype=part.dtype, device=dev)
            dist.all_gather_into_tensor(every, padded, group=self.group)
            out.append(torch.cat([every[r * m:r * m + n] for r, n in enumerate(sizes)]))
        return tuple(out)

    def gather_weights(self, dw: "DeviceWeights") -> "DeviceWeights":
        """All of W from its column shards (shard_w): the ranks' triples concatenated in rank order = (column, row) order,
        because the shards are contiguous column blocks.  A COLLECTIVE: every rank calls it (reading `item_similarity`,
        pickling).  A W that is not sharded is returned as it is."""
        if getattr(dw, "shard", None) is None or self.world_size == 1:
            return dw
        key, val = self._all_gather_triples(dw.cols * dw.n_items + dw.rows, dw.vals)
        return DeviceWeights(key % dw.n_items, key // dw.n_items, val.contiguous(), dw.n_items, dw.f64)

    def _fast_layout(self) -> Optional[Dict[str, Any]]:
        """The fast SPARSE-mode form of this rank's shard (float32 W): feature rows when W has at most 128 non-empty rows
        (popularity-only data), else segments (seg_layout.py).  Built once per W, on the device; None when neither applies
        (float64 W, a backend without the kernels, an empty shard).  Independent of the tiled layout, which SPARSE-mode
        scoring then needs only for the rows whose lists hold an exact score tie (see _local_topk)."""
        W, be = self._W, self.be
        if "fast" in W:
            return W["fast"]
        fast = None
        dw: DeviceWeights = W["dw"]
        torch = be.torch
        if W["col_hi"] > W["col_lo"] and self._fast_dtype_ok() and dw.nnz > 0:
            if getattr(be, "supports_feature_rows", False):
                fr = build_feature_rows_device(torch, dw.rows, dw.cols, dw.vals, W["n_items"], W["col_lo"], W["col_hi"],
                                               tile_cols=self.FR_TILE_COLS)
                if fr is not None:
                    nb = int(be.lib.rtrec_slim_score_fr_scratch_bytes(fr["fr_n_tiles"], fr["fr_tile_cols"]))
                    fr["n_cols"] = int(fr.pop("col_ids_sorted").numel())
                    fr["fr_scratch"] = be.empty((nb,), torch.uint8)      # fr_host: small host copies bench.py prices the kernel's work from
                    fast = fr
            # a W with many rows (item-item structure in the data): the segment layout; the cluster labels that order its
            # columns are kept while W changes little (a mini-batch refits ~3 % of the columns)
            if fast is None:
                fast = W.get("fast_small") or self._seg_form()       # (a small batch may have built it already)
        if fast is not None:
            W["n_active"] = fast["n_cols"]
        W["fast"] = fast
        return fast

    def _fast_dtype_ok(self) -> bool:
        """The fast layouts hold float32 weights and their kernels accumulate float32: right for a float32 W, and usable for a
        float64 W whose values are float32 numbers and all positive (the serial fit's output) through the refine step of
        _local_topk (rtrec_slim_refine_topk_f64)."""
        W = self._W
        if not W["acc_f64"]:
            return True
        return self._f64_refine_mode() != 0

    def _f64_refine_w_ok(self) -> bool:
        """W serves the float64 refine step with the SIGN argument (all weights >= F64_REFINE_MIN_VALUE)."""
        return self._f64_refine_mode() == 1

    def _f64_refine_mode(self) -> int:
        """0: no refine step for this W (lossy upload, switched off, another backend); 1: every weight positive -- relative
        margin (csrc/score_refine.hip); 2: signed weights (positive_only=False, slim_elastic.py:187) -- the absolute slack
        2 (n_u + 2) 2^-24 sum_i |x_ui| max_c |w_ic| per user (_f64_abs_slack), SPARSE mode only."""
        W = self._W
        if "f64_refine" not in W:
            dw: DeviceWeights = W["dw"]
            mode = 0
            if self.f64_refine and isinstance(self.be, HipBackend) and not dw.lossy and dw.nnz > 0:
                mode = 1 if float(dw.vals.min()) >= self.F64_REFINE_MIN_VALUE else 2
                ptr = dw.csc_arrays(self.be.torch)[0]
                W["col_nnz_max"] = int((ptr[1:] - ptr[:-1]).max())
            W["f64_refine"] = mode
        return W["f64_refine"]

    def _f64_abs_slack(self, xb):
        """Signed refine: per row of the batch matrix the bound 2 (n_u + 2) 2^-24 B_u (1 + 1e-6) + 1e-30 with B_u = sum_i
        |x_ui| max_c |w_ic| >= sum |x w| of every column (float64 tensor; cached for the resident X and this W)."""
        torch, W = self.be.torch, self._W
        ptr, col, val = xb
        resident = self._X.get("rptr") is ptr
        # keyed by the identity of the resident row-pointer tensor: set_interactions() replaces X without touching W, and a
        # slack computed for the previous X is too short (new users) or too small (changed ratings) -- ADVICE round 4
        ent = W.get("_f64_slack")
        if resident and ent is not None and ent[0] is ptr:
            return ent[1]
        dw: DeviceWeights = W["dw"]
        if "_row_absmax" not in W:
            rmax = torch.zeros(max(W["n_items"], 1), dtype=torch.float64, device=dw.vals.device)
            rmax.scatter_reduce_(0, dw.rows, dw.vals.abs().double(), "amax", include_self=True)
            W["_row_absmax"] = rmax
        rmax = W["_row_absmax"]
        c64 = col.long()
        inside = c64 < rmax.shape[0]
        contrib = val.abs().double() * torch.where(inside, rmax[c64.clamp(max=rmax.shape[0] - 1)], torch.zeros((), dtype=torch.float64, device=val.device))
        p64 = ptr.long()
        lengths = p64[1:] - p64[:-1]
        n_u = lengths.double()
        try:                # per-row float64 sums (error n_u 2^-53 B_u: far inside the 1e-6 below)
            lo, hi = int(p64[0]), int(p64[-1])
            B = torch.segment_reduce(contrib[lo:hi], "sum", lengths=lengths, unsafe=True)
            err_b = 0.0
        except Exception:   # cumulative sums instead: a difference of two prefixes carries up to 2 N 2^-53 of the TOTAL
            cs = torch.cat([torch.zeros(1, dtype=torch.float64, device=val.device), torch.cumsum(contrib, 0)])
            B = cs[p64[1:]] - cs[p64[:-1]]
            err_b = 2.0 * float(contrib.numel()) * 2.0 ** -53 * float(cs[-1])
        slack = 2.0 * (n_u + 2.0) * 2.0 ** -24 * (B * (1.0 + 1e-6) + err_b) + 1e-30
        if resident:
            W["_f64_slack"] = (ptr, slack)
        return slack

    def _f64_refine_x_ok(self, xb) -> bool:
        """Ratings all >= F64_REFINE_MIN_VALUE (no negative addend, no float32 underflow of a product); cached for the
        resident X."""
        val = xb[2]
        if val.numel() == 0:
            return True
        if self._X.get("rval") is val:
            if "rval_min_ok" not in self._X:
                self._X["rval_min_ok"] = bool(float(val.min()) >= self.F64_REFINE_MIN_VALUE)
            return self._X["rval_min_ok"]
        return bool(float(val.min()) >= self.F64_REFINE_MIN_VALUE)

    def _dense_fill_ok(self, xb) -> bool:
        """rtrec_slim_dense_fill's precondition: weights and ratings all >= F64_REFINE_MIN_VALUE -- every product is a positive
        normal float32 number, so a column the user's row touches has a positive score and every other one exactly +0.0."""
        W = self._W
        if "w_min_ok" not in W:
            dw: DeviceWeights = W["dw"]
            W["w_min_ok"] = bool(not dw.lossy and (dw.nnz == 0 or float(dw.vals.min()) >= self.F64_REFINE_MIN_VALUE))
        return W["w_min_ok"] and self._f64_refine_x_ok(xb)

    def _w_absmax(self) -> Optional[float]:
        """max |w| over the stored weights (NaN when one of them is a NaN; None for an empty W); cached per weights, beside
        w_min_ok."""
        W = self._W
        if "w_absmax" not in W:
            dw: DeviceWeights = W["dw"]
            W["w_absmax"] = float(dw.vals.abs().max()) if dw.nnz else None
        return W["w_absmax"]

    def _x_bound(self, xb) -> Optional[Tuple[int, float]]:
        """(ratings in the longest row, max |x|) of the batch matrix (NaN when a rating is a NaN; None without a rating):
        one reduction and one read-back, cached for the resident X beside rval_min_ok -- its longest row bounds every row
        list scored from it -- and computed once per call for a batch that is not resident."""
        ptr, _col, val = xb
        resident = self._X.get("rval") is val
        if resident and "rval_bound" in self._X:
            return self._X["rval_bound"]
        bound = None
        if val.numel() and ptr.numel() > 1:
            torch = self.be.torch
            n_max, x_max = torch.stack([(ptr[1:] - ptr[:-1]).max().double(), val.abs().max().double()]).tolist()
            bound = (int(n_max), float(x_max))
        if resident:
            self._X["rval_bound"] = bound
        return bound

    def _values_ordinary(self, xb) -> bool:
        """The finite-range PRECONDITION of the fast kernels (include/rtrec_amd.h), checked: n_max * max|x| * max|w| < 2^127."""
        xbound = self._x_bound(xb)
        n_max, x_max = xbound if xbound is not None else (0, None)
        return score_plan.values_ordinary(n_max, x_max, self._w_absmax())

    def _seg_form(self) -> Optional[Dict[str, Any]]:
        """The segment layout of this rank's shard as a layout dict ({"sg": ..., "n_cols": ...}), or None."""
        W, be = self._W, self.be
        dw: DeviceWeights = W["dw"]
        torch = be.torch
        if not (self.use_seg_layout and getattr(be, "supports_seg_layout", False)):
            return None
        from .seg_layout import build_seg_layout_device
        labels = None
        kept = self._sg_labels
        if kept is not None and kept[1] == W["n_items"] and abs(dw.nnz - kept[2]) <= self.SG_RELABEL_FRACTION * max(kept[2], 1):
            labels = kept[0]
        if not self.seg_cluster:
            labels = torch.arange(W["n_items"], dtype=torch.int64, device=dw.rows.device)
        if self.native_seg_builder and hasattr(be, "lib") and dw.nnz < (1 << 27):
            from .seg_layout import build_seg_layout_native, cluster_labels_device
            fresh = labels is None
            if fresh:       # first layout of a model (or W has changed a lot): label propagation over the shard's graph
                sel = (dw.cols >= W["col_lo"]) & (dw.cols < W["col_hi"])
                labels = cluster_labels_device(torch, dw.rows[sel], dw.cols[sel], dw.vals[sel], W["n_items"])
            sg = build_seg_layout_native(be, dw.rows, dw.cols, dw.vals, W["n_items"], W["col_lo"], W["col_hi"], labels)
            labels = None if fresh else labels
        else:
            sg = build_seg_layout_device(torch, dw.rows, dw.cols, dw.vals, W["n_items"], W["col_lo"], W["col_hi"], labels=labels)
        if sg is None:
            return None
        if labels is None:
            self._sg_labels = (sg["sg_labels"], W["n_items"], dw.nnz)
        # zeroed scratch of the heavy pass (long users, one workgroup each); the kernel leaves it zero
        # (kept across layouts of the same size: 130 MB for the ML-20M shape)
        nb = int(be.lib.rtrec_slim_score_sg_scratch_bytes(W["n_items"], sg["sg_n_tiles"], sg["sg_T"]))
        if self._sg_scratch is None or self._sg_scratch.numel() != nb:
            self._sg_scratch = be.zeros((nb,), torch.uint8)
        sg["sg_scratch"] = self._sg_scratch
        return {"sg": sg, "n_cols": int(sg["sg_n_cols"])}

    def _small_batch_layout(self) -> Optional[Dict[str, Any]]:
        """The layout a request-sized batch is scored with: the segment form, whatever the shape of W.  The feature-row kernel
        gives a user to ONE wave that sweeps every tile of W from LDS: 150 us per launch on the ML-20M shape however few
        the users (it is a throughput kernel -- a full pass of 138k users is 1.4 ms).  The segment kernels touch only the
        user's own rows of W, prune tiles by their bounds and give a long user a workgroup: 10-25 us for one user.  So the
        segment form is what a small batch builds (once per W; after a mini-batch the first recommend builds this one
        layout), and the feature-row form waits for the first large pass."""
        W, be = self._W, self.be
        if "fast" in W and (W["fast"] is None or "sg" in W["fast"]):
            return W["fast"]
        if "fast_small" not in W:
            ok = W["col_hi"] > W["col_lo"] and self._fast_dtype_ok() and W["dw"].nnz > 0
            W["fast_small"] = self._seg_form() if ok else None
            if W["fast_small"] is not None:
                W.setdefault("n_active", W["fast_small"]["n_cols"])
        return W["fast_small"] or self._fast_layout()

    def _tile_width(self, compact: bool, top_k: int) -> int:
        """Tile width of the tiled layout: self.tile_cols unless the merge of the per-tile lists (n_tiles * (top_k + 1) <= 1024
        candidates per user) needs wider tiles; capped by what the exact-tie pass fits in LDS (accumulator + first-touch
        word per column)."""
        W = self._W
        acc = 8 if W["acc_f64"] else 4
        max_tile = 256
        while max_tile * 2 * (acc + 4) + 4096 + 16 * (top_k + 64) <= 160 * 1024 and max_tile < 32768:
            max_tile *= 2
        tile = min(self.tile_cols, max_tile)
        width = W["col_hi"] - W["col_lo"]
        if compact and "n_active" in W:
            width = W["n_active"]
        while tile < max_tile and -(-max(width, 1) // tile) * (top_k + 1) > 1024:
            tile *= 2
        return tile

    def _layout(self, compact: bool, top_k: int = 10) -> Optional[Dict[str, Any]]:
        """Tiled layout of this rank's shard (built on the device on first use), with the fast SPARSE-mode form of the
        shard (_fast_layout) merged in when compact."""
        W, be = self._W, self.be
        if compact:
            # (sets n_active, which the tile width of a compacted layout depends on.)  A W with a NaN or an infinite weight
            # never takes a fast pass (score_plan.values_ordinary), so no fast form of it is built either: its builders and
            # their bounds are written for ordinary numbers.  The active columns are counted directly then.
            w_max = self._w_absmax()
            if w_max is None or w_max < score_plan.VALUE_LIMIT:
                self._fast_layout()
            elif "n_active" not in W:
                dw0: DeviceWeights = W["dw"]
                sel = (dw0.cols >= W["col_lo"]) & (dw0.cols < W["col_hi"])
                W["n_active"] = int(be.torch.unique(dw0.cols[sel]).numel())
        tile = self._tile_width(compact, top_k)
        key = (compact, tile)
        if key not in W["layouts"]:
            lay = None
            dw: DeviceWeights = W["dw"]
            torch = be.torch
            if W["col_hi"] > W["col_lo"]:
                lay = build_tiled_w_device(torch, dw.rows, dw.cols, dw.vals, W["n_items"], W["col_lo"], W["col_hi"], tile,
                                           compact=compact, dense_fill=DENSE_ROW_FILL if compact else None)
                if lay is not None and compact:
                    W["n_active"] = lay["n_cols"]
                    fast = W.get("fast")                      # (built above, unless W holds a NaN or an infinite weight)
                    if fast is not None:
                        lay.update({k: v for k, v in fast.items() if k != "n_cols"})
            W["layouts"][key] = lay
        return W["layouts"][key]

    # ------------------------------------------------------------------------------ score
    def _local_topk(self, d_row_ids, n_rows: int, xb, top_k: int, filter_interacted: bool, mode: int,
                    d_col_rank, pad_rows: int = 0, host: bool = False):
        """This rank's lists (ids, scores, float64 scores or None, tie keys, counts) for its columns of W.  A rank that holds
        only PART of the columns (column shards) completes the SPARSE-mode tie key of every entry before the lists travel: two
        columns of different shards can have equal scores without either shard seeing a tie (csrc/score_first_touch.hip)."""
        out = self._local_topk_impl(d_row_ids, n_rows, xb, top_k, filter_interacted, mode, d_col_rank, pad_rows, host)
        be, W = self.be, self._W
        lo, hi = W.get("col_lo", 0), W.get("col_hi", 0)
        if (mode == _native.TOPK_SPARSE and n_rows > 0 and isinstance(be, HipBackend) and hi > lo
                and not (lo == 0 and hi == W["n_items"])):
            ids, _sc, _sc64, aux, cnt = out
            wc_ptr, wc_row, _ = W["dw"].csc_arrays(be.torch)
            be.ops.first_touch_aux(d_row_ids, xb[0], xb[1], n_rows, W["n_items"], wc_ptr, wc_row, top_k, ids, cnt, aux)
        return out

    def _local_topk_impl(self, d_row_ids, n_rows: int, xb, top_k: int, filter_interacted: bool, mode: int,
                         d_col_rank, pad_rows: int = 0, host: bool = False):
        be, W = self.be, self._W
        torch = be.torch
        # ids | scores | counts are views of ONE buffer: a caller that wants them on the host downloads it in one copy
        # (_download: a single-user recommend is three device-to-host round trips otherwise), and the row-sharded path
        # all-gathers it as it is (pad_rows: the buffer is laid out for that many rows, so that every rank's has one size)
        # (host: the caller downloads the lists; the lazy path below then reads its flag counter out of the same copy)
        cap = max(n_rows, int(pad_rows))
        nk = cap * top_k
        flag_words = n_rows + 1 if (host and not pad_rows) else 0
        pack = be.empty((2 * nk + cap + flag_words,), torch.int32)
        ids = pack[:nk].view(cap, top_k)[:n_rows]
        sc = pack[nk:2 * nk].view(torch.float32).view(cap, top_k)[:n_rows]
        cnt = pack[2 * nk:2 * nk + n_rows]
        if cap == n_rows:
            ids._rtrec_pack = pack
        aux = be.empty((n_rows, top_k), torch.int32)
        sc64 = be.empty((n_rows, top_k), torch.float64) if W["acc_f64"] else None
        sparse = mode == _native.TOPK_SPARSE
        hip = isinstance(be, HipBackend)
        # Which kernels serve this call is decided by two pure functions (rtrec_amd/score_plan.py; table-tested on the CPU):
        #   SPARSE mode, float32 W: the fast form of the shard (feature rows / segments).  The tiled layout is then needed only
        #   for the rows whose fast-pass list holds an exact score tie (the exact-tie pass orders those like the reference): with
        #   lazy_tiled it is built when a call first flags such a row -- after a mini-batch the first recommend builds one
        #   layout, not two -- at the price of reading one counter back per call while it does not exist.
        #   DENSE mode (string ids: every column competes, slim_elastic.py:745-778) takes the same fast pass when this rank holds
        #   all of W's columns: a row whose leading top_k scores are all positive is final (positives outrank every zero-score
        #   column, zeros outrank negatives); the kernel flags the others, and every tie (DENSE orders ties by item id), for the
        #   tiled DENSE kernel below.  (A COLUMN SHARD flags nearly every row -- a user's positive scores sit in a few shards --
        #   so it takes the fast pass only when the flagged rows can be completed in place: rtrec_slim_dense_fill.)
        #   float64 W (serial fit): the float32 fast pass for top_k + 1 columns, then the candidates' float64 scores
        #   (rtrec_slim_refine_topk_f64) -- W and X all positive, or (SPARSE) signed with an absolute per-user slack; otherwise
        #   the float64 tiled kernel.
        facts = score_plan.ScoreFacts(
            mode=mode, hip=hip, acc_f64=bool(W["acc_f64"]), top_k=top_k, n_rows=n_rows,
            full_range=(W.get("col_lo", 0) == 0 and W.get("col_hi", 0) == W["n_items"]),
            nonempty_shard=(W.get("col_hi", 0) > W.get("col_lo", 0)),
            dense_fast_on=bool(self.dense_fast), dense_fill_on=bool(self.dense_fill), lazy_tiled=bool(self.lazy_tiled),
            feature_rows_on=bool(self.use_feature_rows), seg_layout_on=bool(self.use_seg_layout),
            seg_supported=bool(getattr(be, "supports_seg_layout", False)),
            dense_fill_ok=lambda: self._dense_fill_ok(xb), f64_w_ok=self._f64_refine_w_ok,
            f64_x_ok=lambda: self._f64_refine_x_ok(xb), f64_refine_mode=self._f64_refine_mode,
            values_ordinary=lambda: self._values_ordinary(xb),
            limits=score_plan.Limits(self.FR_SMALL_BATCH, self.FR_MIN_ROWS, self.FR_MAX_TOP_K, self.SG_MAX_TOP_K))
        req = score_plan.plan_fast_layout(facts)
        fast = None
        if req.want:
            # the segment form: request-sized batches, and any batch whose top_k the feature-row kernel's lists do not hold
            fast = self._small_batch_layout() if req.small else self._fast_layout()
        tiled_key = (sparse, self._tile_width(sparse, top_k))
        plan = score_plan.choose_path(facts, req, has_fr=bool(fast is not None and fast.get("fr_w") is not None),
                                      has_sg=bool(fast is not None and fast.get("sg") is not None),
                                      tiled_exists=tiled_key in W["layouts"])
        out = (ids, sc, sc64, aux, cnt)
        if plan.lazy:             # the fast pass alone; the tiled layout only for the rows it flags (float64 W: always)
            return self._local_topk_lazy(plan, fast, d_row_ids, n_rows, xb, top_k, filter_interacted, mode, d_col_rank, out,
                                         host_pack=pack if flag_words else None)
        lay = self._layout(compact=sparse, top_k=top_k)
        if lay is None:
            ids.fill_(-1); sc.fill_(float("-inf")); aux.zero_(); cnt.zero_()
            if sc64 is not None:
                sc64.fill_(float("-inf"))
            return out
        if plan.use_sg and lay.get("sg") is None:          # a small batch against a feature-row W: its segment form
            lay = dict(lay, sg=fast["sg"])
        self._launch_score(lay, d_row_ids, n_rows, xb, top_k, filter_interacted, mode, d_col_rank, out, plan.use_fr, plan.use_sg,
                           rescored=self.rescored, acc_f64=W["acc_f64"])
        return out

    def _score_workspace(self, need: int):
        """The score kernels' scratch (self._score_ws), grown to at least `need` bytes."""
        if self._score_ws is None or self._score_ws.numel() < need:
            self._score_ws = self.be.empty((need,), self.be.torch.uint8)
        return self._score_ws

    def _launch_score(self, lay, d_row_ids, n_rows: int, xb, top_k: int, filter_interacted: bool, mode: int, d_col_rank, out,
                      use_fr: bool = False, use_sg: bool = False, flagged=None, rescored=None, acc_f64: bool = False,
                      dominant: bool = True, path_suffix: str = "") -> None:
        """THE launch of rtrec_slim_score_topk: `n_rows` rows of the batch `xb` against the layout `lay` into `out` = (ids,
        scores, float64 scores or None, tie keys, counts).  What every launch needs is derived here and nowhere else: the
        scratch, the work order (only when a fast kernel runs; the pattern-grouped one only for the feature-row kernel -- the
        segment kernels rely on the length order), the flag that says which order it is, the diagnostics word.
        `dominant`: the kernel that does the bulk of the call's work -- it alone is bracketed by score_timer (bench.py reads
        it), looks at the diagnostics and names last_score_path; the tiled re-score of a few flagged rows is not."""
        be, W = self.be, self._W
        # (a fast form alone has no tiles of its own: its kernels need the scratch of one)
        ws = self._score_workspace(be.score_workspace_bytes(n_rows, lay.get("n_tiles", 1), top_k))
        args = (n_rows, d_row_ids, xb, W["n_items"], W["col_lo"], lay, d_col_rank, top_k, filter_interacted, mode, acc_f64,
                *out, ws)
        if not isinstance(be, HipBackend):          # the tests' stand-in (tests/cpu_backend.py): the tiled kernel only
            be.score_topk(*args)
            return
        order = self._row_order(d_row_ids, n_rows, xb, lay, allow_grouped=use_fr) if (use_fr or use_sg) else None
        timer = diagnostics = 0
        if dominant:
            timer = self.score_timer
            diagnostics = (self.diagnostics | ((self.fr_users_per_wave & 0xf) << 8) | ((self.sg_heavy_min & 0xfff) << 12)
                           | ((min(self.fr_head_kib, 126) + 1 if self.fr_head_kib >= 0 else 0) << 24))
            self.last_score_path = ("feature_rows" if use_fr else ("segments" if use_sg else "tiled")) + path_suffix
        be.score_topk(*args, timer=timer, diagnostics=diagnostics, use_fr=use_fr, row_order=order, rescored=rescored,
                      row_order_grouped=(order is not None and use_fr and self._order_grouped), use_sg=use_sg,
                      use_sg_heavy=self.use_seg_heavy, flagged=flagged)

    def _rescore_flagged(self, rows_f, d_row_ids, xb, top_k: int, filter_interacted: bool, mode: int, d_col_rank, out) -> None:
        """The flagged rows of a fast pass (`rows_f`: int64 positions in the batch) again, against the tiled layout (built
        now, if this is the first call that needs it) -- its exact-tie pass orders them like the reference -- and scattered
        into `out`; float64 accumulators when `out` carries float64 scores."""
        be, torch = self.be, self.be.torch
        n_f = int(rows_f.numel())
        lay = self._layout(compact=(mode == _native.TOPK_SPARSE), top_k=top_k)
        sub_ids = d_row_ids[rows_f].contiguous() if d_row_ids is not None else rows_f.to(torch.int32)
        f64 = out[2] is not None
        tmp = (be.empty((n_f, top_k), torch.int32), be.empty((n_f, top_k), torch.float32),
               be.empty((n_f, top_k), torch.float64) if f64 else None, be.empty((n_f, top_k), torch.int32),
               be.empty((n_f,), torch.int32))
        self._launch_score(lay, sub_ids, n_f, xb, top_k, filter_interacted, mode, d_col_rank, tmp, acc_f64=f64, dominant=False)
        for dst, src in zip(out, tmp):
            if src is not None:
                dst[rows_f] = src

    F64_REFINE_MIN_VALUE = 1e-18     # ratings and weights at least this large: a product is a normal float32 number

    def _local_topk_lazy(self, plan, fast, d_row_ids, n_rows: int, xb, top_k: int, filter_interacted: bool, mode: int,
                         d_col_rank, out, host_pack=None):
        """The fast pass against `fast` alone, its post-step, and the tiled kernel for the rows the two flag.
        float32 W (Path.FAST): the flagged rows hold an exact score tie.  `host_pack`: the caller downloads the lists (the
        buffer they are views of, flag words at its end), so the flag counter is read out of the same copy.
        float64 W (Path.FAST_F64) with positive float32-valued weights, positive ratings: the float32 fast pass for top_k + 1
        columns, the float64 scores of those candidates (csrc/score_refine.hip), and the float64 tiled kernel for the rows
        either step flags (float32 ties; a top_k-th float64 score too close to what a column outside the list could reach;
        float64 ties).  DENSE mode likewise: its fast pass also flags the rows with fewer than top_k + 1 positive scores (every
        non-zero score is positive here), which the DENSE float64 tiled kernel then scores.  plan.f64_signed (SPARSE): signed
        weights, with the absolute per-user slack of _f64_abs_slack."""
        be, W = self.be, self._W
        torch = be.torch
        ids, sc, sc64, aux, cnt = out
        f64 = plan.path is score_plan.Path.FAST_F64
        k_fast = plan.k_fast
        if f64:
            host_pack = None
            fast_out = (be.empty((n_rows, k_fast), torch.int32), be.empty((n_rows, k_fast), torch.float32), None,
                        be.empty((n_rows, k_fast), torch.int32), be.empty((n_rows,), torch.int32))
            flagged = be.empty((2 * n_rows + 2,), torch.int32)          # a row can be flagged by both steps
        else:
            fast_out = (ids, sc, None, aux, cnt)
            flagged = host_pack[-(n_rows + 1):] if host_pack is not None else be.empty((n_rows + 1,), torch.int32)
        flagged_fast = be.empty((n_rows + 1,), torch.int32) if plan.fill else flagged
        self._launch_score(fast, d_row_ids, n_rows, xb, k_fast, filter_interacted, mode, d_col_rank, fast_out, plan.use_fr,
                           plan.use_sg, flagged=flagged_fast, path_suffix="+f64" if f64 else "")
        if f64:
            ids1, sc1, _, _, cnt1 = fast_out
            wc_ptr, wc_row, wc_val = W["dw"].csc_arrays(torch)
            margin = 2.0 * (W["col_nnz_max"] + 2) * 2.0 ** -24
            be.ops.refine_topk_f64(d_row_ids, xb[0], xb[1], xb[2], n_rows, W["n_items"], wc_ptr, wc_row, wc_val, top_k, ids1, sc1, cnt1,
                                   float(margin), self._f64_abs_slack(xb) if plan.f64_signed else None, ids, sc, sc64, cnt, flagged)
            aux.zero_()
        elif plan.fill:          # DENSE mode: short all-positive lists are completed with the zero-score columns, the rest stays flagged
            be.ops.dense_fill(d_row_ids, xb[0], xb[1], n_rows, int(W["col_lo"]), int(W["col_hi"]), top_k, bool(filter_interacted),
                              ids, sc, aux, cnt, flagged_fast, flagged)
        if host_pack is not None:                # one download: the lists and the counter
            h = host_pack.cpu().numpy()
            n_flag = int(h[-(n_rows + 1)])
            if n_flag == 0:
                ids._rtrec_host = h
        else:
            n_flag = int(flagged[0].item())
        if self.rescored is not None:
            self.rescored.fill_(n_flag)
        if n_flag:
            rows_f = flagged[1:1 + n_flag].long()
            self._rescore_flagged(torch.unique(rows_f) if f64 else rows_f, d_row_ids, xb, top_k, filter_interacted, mode,
                                  d_col_rank, out)
        return out

    ROW_ORDER_MIN = 2048        # batches below this are one or two waves of jobs: nothing to level
    GROUPED_ORDER_MIN = 32768   # the pattern-grouped order (~1 ms to compute, kept per row set) pays for bulk passes only
    # Batches below this many rows go to the tiled-CSR kernel.  Since the feature-row kernel has its 4- and 2-users-per-wave
    # forms (chosen from the batch size inside rtrec_slim_score_topk) it is ahead at every batch size, one user included
    # (tools/score_batch_sweep.py: DESIGN.md section 3.1); the threshold is kept for A/B runs and the tests.
    FR_MIN_ROWS = 1
    SG_RELABEL_FRACTION = 0.2        # the cluster labels that order the segment layout's columns are kept until W's nnz has
                                     # moved by this much (they decide locality only, never a result; label propagation is 3.4 ms)
    FR_SMALL_BATCH = 513              # batches below this many rows are scored from the segment form (_small_batch_layout)
    FR_MAX_TOP_K = 15           # kFrMaxKk - 1 of csrc/score.hip: a list of top_k + 1 entries fits one 16-lane DPP row
    SG_MAX_TOP_K = 63           # kSgMaxKk - 1 of csrc/score_seg.hip.h: the list of top_k + 1 entries is one register across the lanes
    FR_TILE_COLS = 256          # columns per tile of the feature-row layout (128: the narrow kernels, kept for A/B and tests)
    pattern_order = settings.raw("RTREC_AMD_PATTERN_ORDER", "1") != "0"
    rescored = None             # optional int32[1] device tensor: rows the exact-tie pass re-scored in the last call

    def _grouped_order(self, lay, n_rows: Optional[int] = None) -> bool:
        """Pattern-sorted work order with eight consecutive rows per wave: for a feature-row layout of SEVERAL super-tiles,
        whose rows behind the LDS head every wave gathers for itself (C3: 2.37 -> 2.26 ms).  The resident layout (all of W in LDS) keeps the longest-first order dealt out in strides: its waves claim jobs
        on their own, and evenly mixed jobs matter more there than small unions (C2: 0.41 ms against 0.57 ms grouped)."""
        host = (lay or {}).get("fr_host") or {}
        return bool(self.pattern_order and host and not host.get("fr_resident")
                    and (n_rows is None or n_rows >= self.GROUPED_ORDER_MIN))

    ROW_ORDER_GIANTS = 32            # pattern-grouped order: at most this many giant rows are spread over the head ...
    ROW_ORDER_GIANT_LEN = 4096       # ... rows with more entries than this

    def _row_order(self, d_row_ids, n_rows: int, xb, lay=None, allow_grouped: bool = True):
        """Work order for the feature-row kernel (rtrec_score_opts.d_row_order).  Default: the batch's rows by descending
        length.  Layout of several super-tiles (_grouped_order): a wave sweeps -- and, behind the LDS head, fetches --, per tile, the UNION of the rows of W its eight users
        rate, so users with the same rated feature items should share a wave -- the rows are sorted by their feature-row
        pattern as one big integer, the row of W that holds a weight in the most tiles most significant, descending
        (heavy patterns first: the tail of the launch is light): 13 % fewer swept rows on C3.  A function of X, the row set and
        the layout only: kept with the resident X and reused while the same row-id tensor is scored against the same
        layout (bulk scoring, bench.py); small batches go in the order given.
        `allow_grouped=False` (the segment kernels): always the length order -- they are told "longest first" and stop at the
        first short user (a pattern-grouped order there left long users unscored); such a call neither reads
        nor writes the feature-row entries of the cache (its entries carry no layout)."""
        if n_rows < self.ROW_ORDER_MIN:
            self._order_grouped = False
            return None
        torch = self.be.torch
        resident = self._X.get("rptr") is xb[0]
        fr_host = (lay or {}).get("fr_host") if allow_grouped else None
        # One entry per (row-id tensor, layout), matched by IDENTITY: the entry keeps the tensor and the layout alive, so a
        # recycled address can never stand for another row set; a temporary row tensor simply misses.
        # The pattern-grouped order costs milliseconds to compute: a row set gets it the SECOND time it is scored (a caller
        # that keeps its row tensor -- bulk scoring, bench.py); a row set seen once (an API batch) runs in the length order.
        cache = self._X.setdefault("_orders", []) if resident else None
        want_grouped = bool(fr_host is not None and lay.get("fr_map") is not None and self._grouped_order(lay, n_rows))
        seen = None
        self._order_grouped = False
        if cache is not None:
            for ent in cache:
                if (ent[0] is d_row_ids and ent[1] == (None if d_row_ids is None else d_row_ids._version) and ent[2] == n_rows
                        and ent[3] is fr_host):
                    if ent[5] or not want_grouped:
                        self._order_grouped = ent[5]
                        return ent[4]
                    seen = ent
                    break
        grouped = want_grouped and (seen is not None or d_row_ids is None)
        ptr, col = xb[0], xb[1]
        if d_row_ids is None:
            rows = None
            lens = ptr[1:n_rows + 1] - ptr[:n_rows]
        else:
            rows = d_row_ids[:n_rows].long().clamp_(0, ptr.shape[0] - 2)
            lens = ptr[rows + 1] - ptr[rows]
        if not grouped:
            order = torch.argsort(lens, descending=True, stable=True).to(torch.int32)
        else:
            R = int(fr_host["fr_rows"])
            tr = fr_host["fr_rows_of_tile"].view(np.uint64).reshape(-1, 2)
            tiles_of_row = np.array([sum((int(tr[t, f // 64]) >> (f % 64)) & 1 for t in range(tr.shape[0])) for f in range(R)])
            rank = np.empty(R, dtype=np.int64)
            rank[np.argsort(-tiles_of_row, kind="stable")] = np.arange(R)          # 0 = the row in the most tiles
            bit_of_row = torch.from_numpy((R - 1) - rank).to(col.device)              # its bit in the pattern integer
            n_words = -(-R // 60)
            lens64 = lens.long()
            ent_row = torch.repeat_interleave(torch.arange(n_rows, device=col.device), lens64)
            if rows is None:
                ent_col = col[int(ptr[0]):int(ptr[n_rows])].long()
            else:
                within = torch.arange(ent_row.shape[0], device=col.device) - torch.repeat_interleave(
                    torch.cumsum(lens64, 0) - lens64, lens64)
                ent_col = col[ptr[rows].long()[ent_row] + within].long()
            ok = ent_col < lay["fr_map"].shape[0]
            f = torch.full_like(ent_col, -1)
            f[ok] = lay["fr_map"][ent_col[ok]].long()
            keep = f >= 0
            b = bit_of_row[f[keep]]
            words = torch.zeros(n_rows * n_words, dtype=torch.int64, device=col.device)
            words.index_add_(0, ent_row[keep] * n_words + b // 60, torch.ones_like(b) << (b % 60))   # a row's items are distinct
            words = words.view(n_rows, n_words)
            order = torch.arange(n_rows, device=col.device)
            for w in range(n_words):                                  # least significant word first, stable sorts
                order = order[torch.argsort(words[order, w], descending=True, stable=True)]
            order = spread_giant_rows(torch, order, lens64, self.ROW_ORDER_GIANTS, self.ROW_ORDER_GIANT_LEN)
            order = order.to(torch.int32)
        if cache is not None:
            if seen is not None:
                cache[:] = [ent for ent in cache if ent is not seen]       # (by identity: the entries hold tensors)
            if len(cache) >= 32:
                cache.clear()
            cache.append((d_row_ids, None if d_row_ids is None else d_row_ids._version, n_rows, fr_host, order, grouped))
            self._X["_order"] = order          # the most recent one (bench.py's bounds model reads it)
        self._order_grouped = grouped
        return order

    def score_topk_device(self, row_ids: Optional[np.ndarray], n_rows: int, top_k: int, filter_interacted: bool,
                          mode: int, col_rank: Optional[np.ndarray] = None, xb=None, d_rows=None, host: bool = False,
                          candidates: Optional[np.ndarray] = None, with_scores: bool = True):
        """Device tensors (ids, scores, counts) of the GLOBAL top-k for the given rows of X
        (or of the CSR batch `xb` = (ptr, col, val) device tensors).  `d_rows` may pass the row ids
        as a device tensor that is already resident (bench.py reuses it across steps).  Multi-GPU: the exchange of the
        column shards (_score_column_sharded) or of the row shards (_score_row_sharded).
        with_scores=False (row shards): only ids and counts travel -- what `recommend_batch` returns (the reference hands out
        item ids, base.py:188-269) -- 44 instead of 84 bytes per user at k = 10; the score tensor is then None."""
        be = self.be
        if not self._W:
            raise RuntimeError("Model must be fitted before calling batch_recommend.")
        if xb is None:
            xb = self._x_csr()
        up = self._up
        if d_rows is None and row_ids is not None:
            d_rows = up(np.asarray(row_ids, dtype=np.int32))
        if mode == _native.TOPK_CANDIDATES and candidates is not None:
            direct = self._candidates_direct(d_rows, n_rows, xb, top_k, candidates)
            if direct is not None:
                return direct
            if col_rank is None:          # the bulk form: a rank per column of W (the later of two equal candidates wins)
                col_rank = np.full(self._W["n_items"], -1, dtype=np.int32)
                col_rank[np.asarray(candidates, dtype=np.int64)] = np.arange(len(candidates), dtype=np.int32)
        d_rank = up(np.asarray(col_rank, dtype=np.int32)) if col_rank is not None else None
        if self.world_size == 1 and not self.force_exchange:
            ids, sc, sc64, aux, cnt = self._local_topk(d_rows, n_rows, xb, top_k, filter_interacted, mode, d_rank, host=host)
            return ids, sc, cnt
        if d_rows is None:
            d_rows = be.torch.arange(n_rows, dtype=be.torch.int32, device=xb[0].device)
        if self.score_shard == "rows":
            return self._score_row_sharded(d_rows, n_rows, xb, top_k, filter_interacted, mode, d_rank, with_scores)
        return self._score_column_sharded(d_rows, n_rows, xb, top_k, filter_interacted, mode, d_rank)

    def _score_column_sharded(self, d_rows, n_rows: int, xb, k: int, filter_interacted: bool, mode: int, d_rank):
        """score_shard == "columns": every rank scores the rows against its own column shard and packs its per-shard lists
        into ONE int32 record per user -- [scores | ids | first-touch aux | count] (float64 scores in
        front when W is float64).  The exchange is sized for xGMI's point-to-point mesh rather than for
        a switch: an ALL-TO-ALL hands rank r the records of ITS slice of the users from every shard
        (B/G * 124 B from each peer instead of all B * 124 B of an all-gather), merge_topk_kernel merges
        that slice in place through strides, and only the final k-lists (84 B per user) are all-gathered.
        Rows are processed in chunks whose exchanges (RCCL, asynchronous on its own stream) overlap the
        scoring kernel of the next chunk."""
        import torch.distributed as dist
        be = self.be
        torch = be.torch
        G = self.world_size
        f64 = bool(self._W["acc_f64"])
        # chunks exist so that one chunk's exchange overlaps the next chunk's kernel; a chunk must still be large enough to
        # fill the chip (GATHER_CHUNK_ROWS), so passes of up to ~200k rows are one chunk
        per = max(1, int(self.gather_chunk_rows))
        n_chunks = max(1, min(MAX_GATHER_CHUNKS, (n_rows + per // 2) // per))
        per = -(-n_rows // n_chunks)
        lay = exchange_record_layout(k, f64)
        f_ids, f_cnt, width, fwidth = lay["f_ids"], lay["f_cnt"], lay["width"], lay["fwidth"]

        def record(m: int, n_words: int, parts):
            """The column blocks `parts` side by side as [m, n_words] int32 records (a zero pad word where the layout has one)."""
            if sum(int(p.shape[1]) for p in parts) < n_words:
                parts = parts + [torch.zeros((m, 1), dtype=torch.int32, device=parts[0].device)]
            return torch.cat(parts, dim=1)

        res_ids = be.empty((n_rows, k), torch.int32)
        res_sc = be.empty((n_rows, k), torch.float32)
        res_cnt = be.empty((n_rows,), torch.int32)
        pending = []
        for c in range(n_chunks):
            a, b = c * per, min(n_rows, (c + 1) * per)
            m = b - a
            if m <= 0:
                break
            ids, sc, sc64, aux, cnt = self._local_topk(d_rows[a:b], m, xb, k, filter_interacted, mode, d_rank)
            packed = record(m, width, ([sc64.view(torch.int32)] if f64 else []) + [sc.view(torch.int32), ids, aux.view(torch.int32),
                                                                                   cnt.view(m, 1)])
            q = -(-m // G)                      # rows of this chunk each rank merges
            if q * G != m:                      # pad to G equal slices; padded rows carry count 0
                padded = torch.zeros((q * G, width), dtype=torch.int32, device=ids.device)
                padded[:m] = packed
                packed = padded
            recv = be.empty((G * q, width), torch.int32)
            work = dist.all_to_all_single(recv, packed, group=self.group, async_op=True)
            pending.append((a, b, q, recv, packed, work))
        finals = []
        for a, b, q, recv, packed, work in pending:
            work.wait()
            g_ids, g_sc, g_sc64, g_aux, g_cnt = exchange_record_views(torch, recv, G, q, k, f64)   # [source shard, row of my slice, entry]
            s_ids = be.empty((q, k), torch.int32)
            s_sc = be.empty((q, k), torch.float32)
            s_cnt = be.empty((q,), torch.int32)
            be.merge_topk(q, G, k, g_ids, g_sc, g_sc64, g_aux, g_cnt, s_ids, s_sc, s_cnt)
            fin = record(q, fwidth, [s_sc.view(torch.int32), s_ids, s_cnt.view(q, 1)])
            out = be.empty((G * q, fwidth), torch.int32)
            work2 = dist.all_gather_into_tensor(out, fin, group=self.group, async_op=True)
            finals.append((a, b, out, fin, work2))
        for a, b, out, fin, work2 in finals:
            work2.wait()
            m = b - a
            res_sc[a:b] = out[:m, :f_ids].view(torch.float32)
            res_ids[a:b] = out[:m, f_ids:f_cnt]
            res_cnt[a:b] = out[:m, f_cnt]
        return res_ids, res_sc, res_cnt

    def _score_row_sharded(self, d_rows, n_rows: int, xb, k: int, filter_interacted: bool, mode: int, d_rank,
                           with_scores: bool = True):
        """score_shard == "rows": this rank scores rows r, r+G, r+2G, ... of the batch (strided, so that
        every rank gets the same mix of heavy and light users whatever their order) against the whole W
        -- no merge step: its lists are final -- and the final records [k scores | k ids | count] of all
        ranks are all-gathered, 84 B per user at k = 10."""
        import torch.distributed as dist
        be = self.be
        torch = be.torch
        G = self.world_size
        q = -(-n_rows // G)
        # this rank's slice of the batch, kept while the same row tensor is scored again (its work order is cached by it)
        # (matched by the IDENTITY of the row tensor, which the entry keeps alive: an address recycled by the allocator for
        # another call's row ids must never hit -- ADVICE round 2; a temporary tensor simply misses and is sliced again)
        slices = self._X.setdefault("_row_slices", [])
        mine = None
        for ent in slices:
            if ent[0] is d_rows and ent[1] == d_rows._version and ent[2] == (n_rows, self.rank, G):
                mine = ent[3]
        if mine is None:
            mine = d_rows[self.rank::G].contiguous()
            if len(slices) >= 8:
                slices.clear()
            slices.append((d_rows, d_rows._version, (n_rows, self.rank, G), mine))
        m = int(mine.shape[0])
        # Slots (rows of a rank's slice) are cut into chunks so that the all-gather of chunk c (RCCL, asynchronous) runs
        # beside the kernel of chunk c + 1 -- the same overlap the column path has; one blocking gather after the whole
        # local pass used to stand behind the kernel (C4 at 8 ranks: 73.5 MB received per rank after a 0.6 ms kernel,
        # VERDICT round 4).  A chunk keeps at least row_chunk_rows slots: a launch must still fill the chip.
        per = max(1, int(self.row_chunk_rows))
        n_chunks = max(1, min(MAX_GATHER_CHUNKS, q // per))
        bounds = [q * c // n_chunks for c in range(n_chunks + 1)]
        chunk_rows = None                    # this rank's row tensors per chunk: kept with the slice (their work orders are cached by identity)
        for ent in slices:
            if ent[3] is mine and len(ent) > 4 and ent[4][0] == bounds:
                chunk_rows = ent[4][1]
        if chunk_rows is None:
            chunk_rows = [mine[min(bounds[c], m):min(bounds[c + 1], m)] if n_chunks > 1 else mine for c in range(n_chunks)]
            for i_, ent in enumerate(slices):
                if ent[3] is mine:
                    slices[i_] = ent[:4] + ((bounds, chunk_rows),)
        pending = []
        for c in range(n_chunks):
            qc = bounds[c + 1] - bounds[c]
            rows_c = chunk_rows[c]
            mc = int(rows_c.shape[0])
            # every rank's (ids | scores | counts) buffer, laid out for qc slots, is gathered as it is; slots a short slice does
            # not have (global row index >= n_rows) are cut off below, so they may hold anything
            width = (2 * k + 1) * qc
            if mc > 0:
                ids, sc, sc64, aux, cnt = self._local_topk(rows_c, mc, xb, k, filter_interacted, mode, d_rank, pad_rows=qc)
                fin = ids._base if ids._base is not None else ids          # the flat buffer the three are views of
                fin = fin.reshape(-1)
            else:
                fin = be.empty((width,), torch.int32)
            if with_scores:
                out = be.empty((G * width,), torch.int32)
                work = dist.all_gather_into_tensor(out, fin, group=self.group, async_op=(n_chunks > 1))
                pending.append((qc, out, None, fin, (work,)))
            else:           # ids and counts only: two contiguous pieces of the same buffer, two collectives
                out_i, out_c = be.empty((G * qc * k,), torch.int32), be.empty((G * qc,), torch.int32)
                w1 = dist.all_gather_into_tensor(out_i, fin[:qc * k], group=self.group, async_op=(n_chunks > 1))
                w2 = dist.all_gather_into_tensor(out_c, fin[2 * qc * k:2 * qc * k + qc], group=self.group, async_op=(n_chunks > 1))
                pending.append((qc, out_i, out_c, fin, (w1, w2)))
        o_ids_p, o_sc_p, o_cnt_p = [], [], []
        for qc, out, out_c, fin, works in pending:
            for work in works:
                if work is not None:
                    work.wait()
            # slot i of rank p <- row i*G + p of the batch: [slot, rank] order is the batch order
            if with_scores:
                out = out.view(G, (2 * k + 1) * qc)
                o_ids_p.append(out[:, :qc * k].view(G, qc, k).transpose(0, 1).reshape(G * qc, k))
                o_sc_p.append(out[:, qc * k:2 * qc * k].view(G, qc, k).transpose(0, 1).reshape(G * qc, k))
                o_cnt_p.append(out[:, 2 * qc * k:].t().reshape(G * qc))
            else:
                o_ids_p.append(out.view(G, qc, k).transpose(0, 1).reshape(G * qc, k))
                o_cnt_p.append(out_c.view(G, qc).t().reshape(G * qc))
        o_ids = (o_ids_p[0] if n_chunks == 1 else torch.cat(o_ids_p))[:n_rows]
        o_cnt = (o_cnt_p[0] if n_chunks == 1 else torch.cat(o_cnt_p))[:n_rows]
        o_sc = None
        if with_scores:
            o_sc = (o_sc_p[0] if n_chunks == 1 else torch.cat(o_sc_p))[:n_rows].view(torch.float32)
        return o_ids, o_sc, o_cnt

    MAX_TOP_K = 1023            # kMaxTopK of csrc/score.hip
    MAX_MERGE_CANDIDATES = 1024  # per-tile lists of one row the merge kernel takes: n_tiles * (top_k + 1)

    def topk_supported(self, top_k: int, mode: int) -> bool:
        """Whether the fused score + top-k kernels serve this request (rtrec_slim_score_topk's limits);
        callers fall back to score rows from the device + a host selection otherwise."""
        if top_k > self.MAX_TOP_K:
            return False
        compact = mode == _native.TOPK_SPARSE
        W = self._W
        if compact and "n_active" not in W:
            # a shard as wide as ALL its columns is an upper bound: when even that fits the merge, no count is needed
            full = W["col_hi"] - W["col_lo"]
            if -(-max(full, 1) // self._tile_width(False, top_k)) * (top_k + 1) <= self.MAX_MERGE_CANDIDATES:
                return True
        if compact and "n_active" not in W and not W["acc_f64"] and W["dw"].nnz > 0 and W["col_hi"] > W["col_lo"]:
            # the number of columns that hold a weight (what every compacted layout is as wide as): counted from the sorted
            # COO -- no layout is built just to answer this question (the feature-row form alone is 2 ms)
            cols = W["dw"].cols
            inside = cols[(cols >= W["col_lo"]) & (cols < W["col_hi"])]
            W["n_active"] = int((inside[1:] != inside[:-1]).sum()) + 1 if inside.numel() else 0
        if compact and "n_active" not in self._W:
            lay = self._layout(compact=True, top_k=top_k)
            return lay is None or lay["n_tiles"] * (top_k + 1) <= self.MAX_MERGE_CANDIDATES
        width = self._W["n_active"] if compact else self._W["col_hi"] - self._W["col_lo"]
        return -(-max(width, 1) // self._tile_width(compact, top_k)) * (top_k + 1) <= self.MAX_MERGE_CANDIDATES

    CANDS_DIRECT_MAX = 4096             # candidates of a request ranked by rtrec_slim_score_candidates ...
    CANDS_DIRECT_MAX_PAIRS = 1 << 21    # ... while rows x candidates stays a request, not a bulk pass ...
    CANDS_DIRECT_BULK = 1024            # ... and BULK calls with up to this many candidates (round 4): the direct kernel costs
                                        # per (row, candidate column entry), the tiled kernel a pass over all of W whatever the
                                        # list -- all 138,493 c3s users: 20 candidates 2.3 against 18.8 ms, 200: 4.6 / 21.1, 1,000:
                                        # 15.8 / 20.2, 4,096: 84.9 / 20.1, same ids (tools/cands_bench.py)

    def _candidates_direct(self, d_rows, n_rows: int, xb, top_k: int, candidates: np.ndarray):
        """CANDIDATES mode for a request-sized call (csrc/score_cands.hip): the candidates' scores straight from W's CSC
        columns, no pass over all columns and no n_items-sized rank array.  None: not applicable (bulk call, a backend or a
        W it does not serve, several column shards) -- the caller takes the tiled kernel."""
        be, W = self.be, self._W
        n_c = int(len(candidates))
        dw: DeviceWeights = W["dw"]
        if (not isinstance(be, HipBackend) or not self.cands_direct or n_c == 0 or n_c > self.CANDS_DIRECT_MAX
                or (n_rows * n_c > self.CANDS_DIRECT_MAX_PAIRS and n_c > self.CANDS_DIRECT_BULK)
                or (self.world_size > 1 and self.score_shard != "rows")
                or self.force_exchange or dw.lossy or dw.nnz == 0 or top_k > n_c):
            return None
        cands = np.asarray(candidates)
        if int(cands.min()) < 0 or int(cands.max()) >= W["n_items"]:
            return None                       # (the rank-array path raises like the reference's W[:, candidates])
        torch = be.torch
        f64 = bool(W["acc_f64"])
        d_c = be.to_dev_small(cands.astype(np.int32))
        wc_ptr, wc_row, wc_val = dw.csc_arrays(torch)
        nk = n_rows * top_k
        pack = be.empty((2 * nk + n_rows,), torch.int32)
        ids = pack[:nk].view(n_rows, top_k)
        sc = pack[nk:2 * nk].view(torch.float32).view(n_rows, top_k)
        cnt = pack[2 * nk:]
        ids._rtrec_pack = pack
        sc64 = be.empty((n_rows, top_k), torch.float64) if f64 else None
        be.ops.score_candidates(d_rows, xb[0], xb[1], xb[2], n_rows, W["n_items"], wc_ptr, wc_row, wc_val, d_c, top_k, bool(f64),
                                ids, sc, sc64, cnt)
        self.last_score_path = "candidates_direct"
        return ids, sc, cnt

    def _check_rows(self, row_ids: np.ndarray) -> None:
        """Row ids index the resident X: anything outside [0, n_users) would be an out-of-bounds device read
        (the reference's scipy indexing raises IndexError for it)."""
        if len(row_ids) and (int(row_ids.min()) < 0 or int(row_ids.max()) >= self.n_users):
            bad = row_ids[(row_ids < 0) | (row_ids >= self.n_users)]
            raise IndexError(f"row index ({int(bad[0])}) out of range for the resident interaction matrix "
                             f"with {self.n_users} rows")

    def rows_csr(self, row_ids: Sequence[int]) -> sp.csr_matrix:
        """Rows of the resident X as a host CSR (download of just those rows)."""
        row_ids = np.asarray(row_ids, dtype=np.int64)
        self._check_rows(row_ids)
        torch = self.be.torch
        X = self._X
        d_rows = self.be.to_dev(row_ids)
        beg, end = X["rptr"][d_rows].long(), X["rptr"][d_rows + 1].long()
        cnt = end - beg
        indptr = np.zeros(len(row_ids) + 1, dtype=np.int64)
        indptr[1:] = np.cumsum(cnt.cpu().numpy())
        total = int(indptr[-1])
        if total:
            off = torch.arange(total, device=d_rows.device) - torch.repeat_interleave(
                torch.as_tensor(indptr[:-1], device=d_rows.device), cnt) + torch.repeat_interleave(beg, cnt)
            cols, vals = X["rcol"][off].cpu().numpy(), X["rval"][off].cpu().numpy()
        else:
            cols, vals = np.empty(0, np.int32), np.empty(0, np.float32)
        return sp.csr_matrix((vals, cols, indptr), shape=(len(row_ids), self.n_items))

    def recommend_rows(self, row_ids: Sequence[int], top_k: int = 10, filter_interacted: bool = True,
                       mode: int = _native.TOPK_SPARSE, col_rank: Optional[np.ndarray] = None,
                       candidates: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Top-k for rows of the resident X.  Returns numpy (ids[B,k], scores[B,k], counts[B]).  CANDIDATES mode: either the
        rank array `col_rank` (n_items entries, -1 = not a candidate) or the list `candidates` itself."""
        row_ids = np.asarray(row_ids, dtype=np.int64)
        if len(row_ids) == 0:
            return self._empty_lists(top_k)
        self._check_rows(row_ids)
        row_ids = row_ids.astype(np.int32)
        return self._download(*self.score_topk_device(row_ids, len(row_ids), top_k, filter_interacted, mode, col_rank, host=True,
                                                      candidates=candidates))

    @staticmethod
    def _download(ids, sc, cnt) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids, scores, counts) device tensors -> numpy; one copy when they are the views _local_topk hands out."""
        pack = getattr(ids, "_rtrec_pack", None)
        if pack is None:
            return ids.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()
        n, k = ids.shape
        h = getattr(ids, "_rtrec_host", None)
        if h is None:
            h = pack.cpu().numpy()
        return h[:n * k].reshape(n, k), h[n * k:2 * n * k].view(np.float32).reshape(n, k), h[2 * n * k:2 * n * k + n]

    def recommend_csr(self, Xb: sp.csr_matrix, top_k: int = 10, filter_interacted: bool = True,
                      mode: int = _native.TOPK_SPARSE, col_rank: Optional[np.ndarray] = None,
                      candidates: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Top-k for the rows of a host CSR batch (the SLIMElastic.recommend_batch boundary)."""
        B = Xb.shape[0]
        if B == 0:
            return self._empty_lists(top_k)
        return self._download(*self.score_topk_device(None, B, top_k, filter_interacted, mode, col_rank, xb=self._upload_csr(Xb),
                                                      candidates=candidates))

    @staticmethod
    def _empty_lists(top_k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids, scores, counts) of a call without rows."""
        return np.empty((0, top_k), np.int32), np.empty((0, top_k), np.float32), np.empty((0,), np.int32)

    def _upload_csr(self, Xb: sp.csr_matrix):
        """A host CSR batch as the (ptr, col, val) device tensors the score kernels read (sorted indices, int32 / float32)."""
        be = self.be
        if not Xb.has_sorted_indices:
            Xb = Xb.sorted_indices()
        return (be.to_dev(np.asarray(Xb.indptr, dtype=np.int32)), be.to_dev(np.asarray(Xb.indices, dtype=np.int32)),
                be.to_dev(np.asarray(Xb.data, dtype=np.float32)))

    # ------------------------------------------------------------------------------ score vectors
    def predict_csr(self, Xb: sp.csr_matrix) -> np.ndarray:
        """Dense score rows Xb . W (float32, or float64 for a float64 W) for a host CSR batch:
        the SLIMElastic.predict* boundary.  [B, n_items]; with several ranks each computes its own
        column block and the blocks are concatenated on the host."""
        be, W = self.be, self._W
        if not W:
            raise RuntimeError("Model must be fitted before calling predict.")
        torch = be.torch
        B = Xb.shape[0]
        xb = self._upload_csr(Xb)
        lay = self._layout(compact=False)
        dt = torch.float64 if W["acc_f64"] else torch.float32
        n_local = W["col_hi"] - W["col_lo"]
        out = be.zeros((B, max(n_local, 1)), dt)
        if lay is not None and B > 0:
            be.score_rows(B, None, xb, W["n_items"], W["col_lo"], lay, W["acc_f64"], out)
        block = out.cpu().numpy()[:, :n_local]
        if self.world_size == 1 or self.score_shard == "rows":      # rows mode: W is not sharded
            return block
        import torch.distributed as dist
        parts: List[Any] = [None] * self.world_size
        dist.all_gather_object(parts, block, group=self.group)
        return np.concatenate(parts, axis=1)

    # ------------------------------------------------------------------------------ similar
    def similar_items(self, queries: Sequence[int], top_k: int = 10) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        if not self._W:
            raise RuntimeError("Model must be fitted before calling similar_items.")
        q = np.asarray(queries, dtype=np.int32)
        if len(q) == 0:
            return self._empty_lists(top_k)
        ids, sc, cnt = self.similar_items_device(q, top_k)
        return ids.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()

    def similar_items_device(self, queries: np.ndarray, top_k: int = 10):
        """similar_items() where it leaves its answer: device tensors (ids[n, top_k] int32, scores[n, top_k] float32,
        count[n] int32) for the internal item ids `queries` (at least one, all inside the catalogue)."""
        be, W = self.be, self._W
        if not W:
            raise RuntimeError("Model must be fitted before calling similar_items.")
        torch = be.torch
        q = np.asarray(queries, dtype=np.int32)
        n = len(q)
        d_q = be.to_dev(q)
        ids = be.empty((n, top_k), torch.int32)
        sc = be.empty((n, top_k), torch.float32)
        cnt = be.empty((n,), torch.int32)
        be.similar_topk(d_q, self._w_csc(), top_k, ids, sc, cnt)
        if getattr(W["dw"], "shard", None) is not None and self.world_size > 1:
            # W is column-sharded: column j is held by its owner alone ("similar_items(j) is served by the owner of
            # column j"); every rank answers its own queries and one all-gather of [n, 2k + 1] words brings them together
            import torch.distributed as dist
            pack = torch.cat([ids, sc.view(torch.int32), cnt.view(n, 1)], dim=1).contiguous()
            allp = be.empty((self.world_size * n, 2 * top_k + 1), torch.int32)
            dist.all_gather_into_tensor(allp, pack, group=self.group)
            bounds = np.array([shard_bounds(W["n_items"], self.world_size, r)[1] for r in range(self.world_size)])
            owner = np.searchsorted(bounds, np.clip(q.astype(np.int64), 0, W["n_items"] - 1), side="right")
            pick = be.to_dev(owner.astype(np.int64) * n + np.arange(n, dtype=np.int64))
            mine = allp[pick]
            ids, sc, cnt = mine[:, :top_k], mine[:, top_k:2 * top_k].view(torch.float32), mine[:, 2 * top_k]
        return ids, sc, cnt

    # ------------------------------------------------------------------------------ explanations
    EXPLAIN_MAX_LIST = 64       # list_k / top_m limits of rtrec_slim_explain_topk
    EXPLAIN_MAX_TOP_M = 32

    # The request calls below read the whole of W on this rank, with the float32 values the scores were computed from (a
    # float64 W whose values are float32 numbers is served with those numbers).  Per call: who needs it, what to do with the
    # gathered model, what would not be exact.
    _WHOLE_W = {
        "explain": ("explanations need", "explain", "explanations are exact float32 products"),
        "score_pairs": ("pair scores need", "score_pairs", "pair scores are exact float32 products"),
        "recommend_users": ("an audience needs", "serve audiences", "audience scores are exact float32 sums"),
        "diversify": ("diversified lists need", "diversify", "similarities are W's float32 values"),
        "list_quality": ("list quality needs", "measure the lists", "similarities are W's float32 values"),
        # (no third entry: the ranks are counted over the score rows this W gives, in float64 for a float64 W, whatever was uploaded)
        "catalogue_ranks": ("catalogue ranks need", "rank", None),
        "blend": ("blended lists need", "blend", "SLIM's side of a blend is its float32 scores"),
        "similar_hybrid": ("hybrid similar items need", "serve them", "SLIM's side of the blend is W's float32 values"),
    }

    def _whole_w(self, call: str) -> DeviceWeights:
        """The W that `call` (a key of _WHOLE_W) reads, or the reason why this engine cannot serve it."""
        needs, verb, exact = self._WHOLE_W[call]
        if not self._W:
            raise RuntimeError(f"Model must be fitted before calling {call}.")
        dw: DeviceWeights = self._W["dw"]
        if getattr(dw, "shard", None) is not None and self.world_size > 1:
            raise ValueError(f"{needs} the whole of W on this rank, and W is column-sharded (shard_w): "
                             f"gather it with gather_item_similarity() and {verb} from the gathered model")
        if dw.lossy and exact is not None:
            raise ValueError(f"{exact}; this W was uploaded from a float64 matrix whose values "
                             "are not float32 numbers (DeviceWeights.lossy)")
        return dw

    def _w_csc(self) -> Dict[str, Any]:
        """W's CSC view as the dict the backend's request methods take."""
        cptr, crow, cval = self._W["dw"].csc_arrays(self.be.torch)
        return {"cptr": cptr, "crow": crow, "cval": cval}

    def _x_csr(self):
        """The resident X as the (ptr, col, val) device tensors an `xb` argument stands for."""
        return self._X["rptr"], self._X["rcol"], self._X["rval"]

    @staticmethod
    def _host_lists(item_ids, scores=None, counts=None, n_rows: Optional[int] = None,
                    shape_error: str = "item_ids (and scores) must be [B, k] arrays of one shape"):
        """The lists a caller brings, as the kernels take them: contiguous int32 ids [B, k], float32 scores of that shape (None
        stays None) and int32 counts [B] (default k).  `n_rows`: the B the caller expects; `shape_error`: what to say when
        the ids or the scores do not have the shape."""
        item_ids = np.ascontiguousarray(item_ids, dtype=np.int32)
        if scores is not None:
            scores = np.ascontiguousarray(scores, dtype=np.float32)
        if (item_ids.ndim != 2 or (n_rows is not None and item_ids.shape[0] != n_rows)
                or (scores is not None and scores.shape != item_ids.shape)):
            raise ValueError(shape_error)
        B, k = item_ids.shape
        counts = np.full(B, k, dtype=np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
        if counts.shape != (B,):
            raise ValueError("counts must hold one entry per row")
        return item_ids, scores, counts

    @staticmethod
    def _rows32(row_ids, n_x: int) -> np.ndarray:
        """`row_ids` as int32, -1 (no row) for a row outside the n_x rows of X."""
        rows = np.asarray(row_ids, dtype=np.int64)
        return np.where((rows >= 0) & (rows < n_x), rows, -1).astype(np.int32)

    def _upload_lists(self, row_ids, item_ids, counts, xb):
        """The host side of explain_rows / score_pairs_rows: (B, k, device rows, device ids, device counts) for the lists
        `item_ids` [B, k] of the rows `row_ids`; counts default to k, a row outside the matrix becomes -1 (no row)."""
        row_ids = np.asarray(row_ids, dtype=np.int64)
        item_ids, _, counts = self._host_lists(item_ids, None, counts, len(row_ids), "item_ids must be [len(row_ids), k]")
        B, k = item_ids.shape
        rows32 = self._rows32(row_ids, self.n_users if xb is None else int(xb[0].shape[0]) - 1)
        return B, k, self._up(rows32), self._up(item_ids), self._up(counts)

    def explain_device(self, d_rows, n_rows: int, xb, ids, counts, top_m: int):
        """Device tensors (reason_items[n_rows, k, top_m], contributions[same], support[n_rows, k]) for the lists `ids`
        [n_rows, k] / `counts` [n_rows] (int32 device tensors, e.g. what score_topk_device returned: they never leave HBM) of
        the rows `d_rows` (int32 device tensor, or None = rows 0 .. n_rows-1) of `xb` = (ptr, col, val) device tensors (None:
        the resident X).  The contract is the comment of rtrec_slim_explain_topk in include/rtrec_amd.h.  Every rank that
        holds the whole W answers locally: there is no collective."""
        be, torch = self.be, self.be.torch
        dw = self._whole_w("explain")
        k = int(ids.shape[-1])
        if not 1 <= k <= self.EXPLAIN_MAX_LIST or not 1 <= int(top_m) <= self.EXPLAIN_MAX_TOP_M:
            raise ValueError(f"explain: lists of 1..{self.EXPLAIN_MAX_LIST} items and top_m in 1..{self.EXPLAIN_MAX_TOP_M} "
                             f"are supported, got {k} and {top_m}")
        if xb is None:
            xb = self._x_csr()
        items = be.empty((n_rows, k, int(top_m)), torch.int32)
        contrib = be.empty((n_rows, k, int(top_m)), torch.float32)
        support = be.empty((n_rows, k), torch.int32)
        if n_rows == 0:
            return items, contrib, support
        be.explain_topk(d_rows, xb, dw.n_items, self._w_csc(), ids.contiguous(), counts.contiguous(), k, int(top_m), items, contrib,
                        support)
        return items, contrib, support

    def explain_rows(self, row_ids: Sequence[int], item_ids: np.ndarray, counts: Optional[np.ndarray] = None, top_m: int = 3,
                     xb=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """explain_device for lists the caller brings: numpy (reason_items[B, k, top_m], contributions, support[B, k]) for
        `item_ids` [B, k] (-1 = no item) of the rows `row_ids` of the resident X -- or of the device CSR batch `xb`.  A row id
        outside the matrix is a user without a row: support 0 everywhere."""
        B, k, d_rows, d_ids, d_counts = self._upload_lists(row_ids, item_ids, counts, xb)
        if B == 0:
            self._whole_w("explain")
            return (np.empty((0, k, top_m), np.int32), np.empty((0, k, top_m), np.float32), np.empty((0, k), np.int32))
        out = self.explain_device(d_rows, B, xb, d_ids, d_counts, top_m)
        return tuple(t.cpu().numpy() for t in out)

    # ------------------------------------------------------------------------------ rerank: per-user candidate lists
    PAIRS_MAX_LIST = 1024       # list_k limit of rtrec_slim_score_pairs

    def score_pairs_device(self, d_rows, n_rows: int, xb, ids, counts, top_k: int = 0, filter_interacted: bool = False,
                           waves_per_row: int = 0):
        """Device tensors (scores[n_rows, k] float32, support[n_rows, k] int32, order[n_rows, top_k] int32, count[n_rows] int32)
        for the lists `ids` [n_rows, k] / `counts` [n_rows] (int32 device tensors: lists other kernels produced never leave HBM)
        of the rows `d_rows` (int32 device tensor, or None = rows 0 .. n_rows-1) of `xb` = (ptr, col, val) device tensors (None:
        the resident X).  score = the float32 sum of x_uj * w_ji over the common j in ascending j, support = their number (-1:
        an empty position), order = the list POSITIONS by rank (score descending, the later position first among equal
        scores; NaN scores and, with `filter_interacted`, items stored in the row do not compete), -1 behind count.  The
        contract is the comment of rtrec_slim_score_pairs in include/rtrec_amd.h.  `top_k == 0`: scores and supports only, and
        lists longer than 1024 are worked through in column chunks; ranking serves lists of up to 1024.  The results stay in
        HBM.  Every rank that holds the whole W answers locally: there is no collective."""
        be, torch = self.be, self.be.torch
        dw = self._whole_w("score_pairs")
        k, top_k, n_rows = int(ids.shape[-1]), int(top_k), int(n_rows)
        if top_k > 0 and k > self.PAIRS_MAX_LIST:
            raise ValueError(f"score_pairs ranks lists of up to {self.PAIRS_MAX_LIST} items, got {k}: longer lists are scored "
                             "with top_k=0 only")
        if not 0 <= top_k <= max(k, 0):
            raise ValueError(f"score_pairs: top_k must lie in 0..{k} (the list length), got {top_k}")
        scores = be.empty((n_rows, k), torch.float32)
        support = be.empty((n_rows, k), torch.int32)
        order = be.empty((n_rows, top_k), torch.int32)
        count = be.zeros((n_rows,), torch.int32)
        if n_rows == 0 or k == 0:
            return scores, support, order, count
        if xb is None:
            xb = self._x_csr()
        W = self._w_csc()
        if k <= self.PAIRS_MAX_LIST:
            be.score_pairs(d_rows, xb, dw.n_items, W, ids.contiguous(), counts.contiguous(), k, top_k, bool(filter_interacted),
                           scores, support, order, count, waves_per_row=waves_per_row)
            return scores, support, order, count
        for c0 in range(0, k, self.PAIRS_MAX_LIST):                      # top_k == 0: column chunks of the kernel's list length
            c1 = min(k, c0 + self.PAIRS_MAX_LIST)
            sc, su = be.empty((n_rows, c1 - c0), torch.float32), be.empty((n_rows, c1 - c0), torch.int32)
            be.score_pairs(d_rows, xb, dw.n_items, W, ids[:, c0:c1].contiguous(), (counts - c0).clamp(0, c1 - c0).to(torch.int32),
                           c1 - c0, 0, False, sc, su, order, count, waves_per_row=waves_per_row)
            scores[:, c0:c1], support[:, c0:c1] = sc, su
        return scores, support, order, count

    def score_pairs_rows(self, row_ids: Sequence[int], item_ids: np.ndarray, counts: Optional[np.ndarray] = None, top_k: int = 0,
                         filter_interacted: bool = False, xb=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """score_pairs_device for lists the caller brings: numpy (scores[B, k], support[B, k], order[B, top_k], count[B]) for
        `item_ids` [B, k] (-1 = no item) of the rows `row_ids` of the resident X -- or of the device CSR batch `xb`.  A row id
        outside the matrix is a user without a row: score 0 and support 0 for every valid item."""
        B, _, d_rows, d_ids, d_counts = self._upload_lists(row_ids, item_ids, counts, xb)
        out = self.score_pairs_device(d_rows, B, xb, d_ids, d_counts, top_k, filter_interacted)
        return tuple(t.cpu().numpy() for t in out)

    # ------------------------------------------------------------------------------ diversified lists (greedy MMR over W)
    DIVERSE_MAX_LIST = 1024     # list_k limit of rtrec_slim_diversify_lists

    def diversify_device(self, ids, scores, counts, keep: int, lam: float, waves_per_row: int = 0):
        """Device tensors (order[n_rows, keep] int32, value[n_rows, keep] float32, penalty[n_rows, keep] float32, count[n_rows]
        int32) for the lists `ids` [n_rows, k] int32 / `scores` [n_rows, k] float32 / `counts` [n_rows] int32 (device tensors,
        e.g. what score_topk_device returned: they never leave HBM): the greedy selection that trades lam * score against
        (1 - lam) * the largest similarity to what is already chosen, similarity = max(|W[a, b]|, |W[b, a]|).  order holds list
        POSITIONS, value / penalty the step's value and penalty of the chosen entry, -1 / -inf / -inf behind count.  The
        contract is the comment of rtrec_slim_diversify_lists in include/rtrec_amd_ext.h.  Every rank that holds the whole W
        answers locally: there is no collective."""
        be, torch = self.be, self.be.torch
        dw = self._whole_w("diversify")
        n_rows, k, keep, lam = int(ids.shape[0]), int(ids.shape[-1]), int(keep), float(lam)
        if not 1 <= k <= self.DIVERSE_MAX_LIST or not 1 <= keep <= k:
            raise ValueError(f"diversify: lists of 1..{self.DIVERSE_MAX_LIST} items and keep in 1..the list length are "
                             f"supported, got {k} and {keep}")
        if not 0.0 <= lam <= 1.0:                                         # (a NaN fails both compares)
            raise ValueError(f"diversify: lam must lie in [0, 1], got {lam}")
        if tuple(scores.shape) != (n_rows, k) or int(counts.numel()) != n_rows:
            raise ValueError("diversify: scores must have the shape of ids, counts one entry per row")
        order = be.empty((n_rows, keep), torch.int32)
        value = be.empty((n_rows, keep), torch.float32)
        penalty = be.empty((n_rows, keep), torch.float32)
        count = be.zeros((n_rows,), torch.int32)
        if n_rows == 0:
            return order, value, penalty, count
        be.diversify_lists(dw.n_items, self._w_csc(), ids.contiguous(), scores.contiguous(), counts.contiguous(), k, keep, lam,
                           order, value, penalty, count, waves_per_row=waves_per_row)
        return order, value, penalty, count

    def diversify_lists(self, item_ids: np.ndarray, scores: np.ndarray, counts: Optional[np.ndarray] = None, keep: int = 10,
                        lam: float = 0.7) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """diversify_device for lists the caller brings: numpy (order[B, keep], value, penalty, count[B]) for `item_ids` [B, k]
        (-1 or an id outside W = an empty position) with the base scores `scores` [B, k]; counts default to k."""
        item_ids, scores, counts = self._host_lists(item_ids, scores, counts)
        out = self.diversify_device(self._up(item_ids), self._up(scores), self._up(counts), keep, lam)
        return tuple(t.cpu().numpy() for t in out)

    # ------------------------------------------------------------------------------ list quality (what a list looks like, over W)
    QUALITY_MAX_LIST = 1024     # list_k limit of rtrec_slim_list_quality

    def item_novelty_device(self):
        """The novelty table of the resident X for W's items, a float32 device tensor [W's n_items]: self-information
        log2(n_users) - log2(max(pop_i, 1)), pop_i = the stored entries of column i of X (utils.metrics.novelty_weights: numpy
        in float64, rounded once).  Columns X has beyond W are cut, columns W has beyond X count as never seen -- the way
        audience_device treats cptr.  Built once per (X, W's width): it is cached on the X dict like the other tensors derived
        from X, so the next set_interactions drops it."""
        from .utils.metrics import novelty_weights
        dw = self._whole_w("list_quality")
        if not self._X:
            raise RuntimeError("set_interactions() must be called before item_novelty_device()")
        cache = self._X.setdefault("item_novelty", {})
        if dw.n_items not in cache:
            if "col_nnz" in self._X:
                pop = np.asarray(self._X["col_nnz"], dtype=np.int64)
            else:                       # only the CSR orientation is resident: one count of its column ids on the device
                rcol = self._X["rcol"]
                pop = self.be.torch.bincount(rcol.to(self.be.torch.int64), minlength=self.n_items).cpu().numpy().astype(np.int64)
            cache[dw.n_items] = self._up(novelty_weights(pop, self.n_users, dw.n_items))
        return cache[dw.n_items]

    def list_quality_device(self, ids, counts, item_weight=None, exposure=None, waves_per_row: int = 0):
        """Device tensors (n[n_rows] int32, sim_sum[n_rows] float32, linked[n_rows] int32, weight_sum[n_rows] float32) for the
        lists `ids` [n_rows, k] int32 / `counts` [n_rows] int32 (device tensors, e.g. what score_topk_device or the gather
        behind diversify_device left: they never leave HBM): the counted positions of each list (inside W, below counts, every
        item once), the two-level float32 sum of similarity = max(|W[a, b]|, |W[b, a]|) over its pairs, the pairs with a
        similarity above 0, and the sum of `item_weight` [W's n_items] float32 (None: +0).  `exposure` [W's n_items] int32
        (None: not kept) gets 1 added per counted position and is never zeroed, so it accumulates over calls.  The contract is
        the comment of rtrec_slim_list_quality in include/rtrec_amd_ext.h.  Every rank that holds the whole W answers locally:
        there is no collective."""
        be, torch = self.be, self.be.torch
        dw = self._whole_w("list_quality")
        n_rows, k = int(ids.shape[0]), int(ids.shape[-1])
        if ids.dim() != 2 or not 1 <= k <= self.QUALITY_MAX_LIST:
            raise ValueError(f"list_quality: lists of 1..{self.QUALITY_MAX_LIST} items are supported, got {k}")
        if int(counts.numel()) != n_rows:
            raise ValueError("list_quality: counts must hold one entry per row")
        for name, t in (("item_weight", item_weight), ("exposure", exposure)):
            if t is not None and int(t.numel()) != dw.n_items:
                raise ValueError(f"list_quality: {name} must hold one entry per item of W ({dw.n_items}), got {int(t.numel())}")
        n = be.zeros((n_rows,), torch.int32)
        sim_sum = be.zeros((n_rows,), torch.float32)
        linked = be.zeros((n_rows,), torch.int32)
        weight_sum = be.zeros((n_rows,), torch.float32)
        if n_rows == 0:
            return n, sim_sum, linked, weight_sum
        be.list_quality(dw.n_items, self._w_csc(), ids.contiguous(), counts.contiguous(), k, item_weight, exposure, n, sim_sum, linked,
                        weight_sum, waves_per_row=waves_per_row)
        return n, sim_sum, linked, weight_sum

    def list_quality_lists(self, item_ids: np.ndarray, counts: Optional[np.ndarray] = None, item_weight: Optional[np.ndarray] = None,
                           novelty: bool = False, with_exposure: bool = True, waves_per_row: int = 0):
        """list_quality_device for lists the caller brings: numpy (n[B], sim_sum[B], linked[B], weight_sum[B], exposure[W's
        n_items] or None) for `item_ids` [B, k] (-1 or an id outside W = an empty position); counts default to k,
        `item_weight` [W's n_items] float32 or None; `novelty=True` weighs with item_novelty_device() instead."""
        item_ids, _, counts = self._host_lists(item_ids, None, counts)
        dw = self._whole_w("list_quality")
        if novelty and item_weight is not None:
            raise ValueError("list_quality: pass item_weight or novelty=True, not both")
        d_w = self.item_novelty_device() if novelty else None if item_weight is None else self._up(np.ascontiguousarray(item_weight, dtype=np.float32))
        d_exp = self.be.zeros((dw.n_items,), self.be.torch.int32) if with_exposure else None
        out = self.list_quality_device(self._up(item_ids), self._up(counts), d_w, d_exp, waves_per_row)
        return tuple(t.cpu().numpy() for t in out) + (d_exp.cpu().numpy() if with_exposure else None,)

    # ------------------------------------------------------------------------------ blended lists (two lists per row, one union)
    BLEND_MAX_LIST = 1024       # ka / kb limit of rtrec_slim_blend_lists

    def blend_device(self, a_ids, a_scores, a_counts, b_ids, b_scores, b_counts, keep: int, weight_b: float = 1.0,
                     contacts: bool = False, k: float = 2.0, mnz: bool = False, d_rows=None, xb=None, cn=None,
                     waves_per_row: int = 0):
        """Device tensors (ids[n_rows, keep] int32, value[n_rows, keep] float32, source[n_rows, keep] int32, count[n_rows] int32)
        for the union of the lists A = `a_ids` [n_rows, ka] int32 / `a_scores` [n_rows, ka] float32 / `a_counts` [n_rows] int32
        (another scorer's) and B in the same form (SLIM's, e.g. what score_topk_device returned: it never leaves HBM): each list
        min-max normalised in float32, B's part weighted by `weight_b` or -- with `contacts` -- by (float32)(2 n / (n + k)) with n
        the contacts of the row's user with the item, added into the union by item id, ranked by value with the earlier entry
        first among equal values; `mnz` doubles what stands in both lists.  source is 1 (only A), 2 (only B) or 3; -1 / -inf / 0
        stand behind count.  With `contacts`, `d_rows` (int32 device tensor, None = rows 0 .. n_rows-1) names the row of
        `xb` = (ptr, col, val) device tensors (None: the resident X) behind each list, and `cn` = (ptr, col, val) int32 device
        tensors (or None) is the count CSR over the same rows: a stored count wins, otherwise n is 1 for an item the row stores
        and 0 for any other.  The contract is the comment of rtrec_slim_blend_lists in include/rtrec_amd_ext.h.  W is not read
        (only its width, the catalogue): every rank answers locally."""
        be, torch = self.be, self.be.torch
        if not self._W:
            raise RuntimeError("Model must be fitted before calling blend.")
        n_items = int(self._W["n_items"])
        n_rows, ka, kb, keep = int(a_ids.shape[0]), int(a_ids.shape[-1]), int(b_ids.shape[-1]), int(keep)
        if a_ids.dim() != 2 or b_ids.dim() != 2 or not 1 <= ka <= self.BLEND_MAX_LIST or not 1 <= kb <= self.BLEND_MAX_LIST:
            raise ValueError(f"blend: two lists of 1..{self.BLEND_MAX_LIST} items per row are supported, got {ka} and {kb}")
        if not 1 <= keep <= ka + kb:
            raise ValueError(f"blend: keep must lie in 1..{ka + kb} (both list lengths together), got {keep}")
        if not float(weight_b) >= 0.0 or not float(k) >= 0.0:                # (a NaN fails the compare)
            raise ValueError(f"blend: the weight and k must not be negative or NaN, got {weight_b} and {k}")
        if (tuple(a_scores.shape) != (n_rows, ka) or tuple(b_ids.shape) != (n_rows, kb) or tuple(b_scores.shape) != (n_rows, kb)
                or int(a_counts.numel()) != n_rows or int(b_counts.numel()) != n_rows):
            raise ValueError("blend: scores must have the shape of their ids, both lists one row per row, counts one entry per row")
        ids = be.empty((n_rows, keep), torch.int32)
        value = be.empty((n_rows, keep), torch.float32)
        source = be.empty((n_rows, keep), torch.int32)
        count = be.zeros((n_rows,), torch.int32)
        if n_rows == 0:
            return ids, value, source, count
        if contacts and xb is None:
            if not self._X:
                raise RuntimeError("set_interactions() must be called before blend with contacts")
            xb = self._x_csr()
        be.blend_lists(n_items, a_ids.contiguous(), a_scores.contiguous(), a_counts.contiguous(), ka, b_ids.contiguous(),
                       b_scores.contiguous(), b_counts.contiguous(), kb, keep, float(weight_b), bool(contacts), float(k), bool(mnz),
                       d_rows if contacts else None, xb if contacts else None, cn if contacts else None, ids, value, source, count,
                       waves_per_row=waves_per_row)
        return ids, value, source, count

    def blend_lists(self, a_ids: np.ndarray, a_scores: np.ndarray, b_ids: np.ndarray, b_scores: np.ndarray,
                    a_counts: Optional[np.ndarray] = None, b_counts: Optional[np.ndarray] = None, keep: int = 10, weight_b: float = 1.0,
                    mnz: bool = False, row_ids: Optional[Sequence[int]] = None, contact_counts: Optional[sp.csr_matrix] = None,
                    k: float = 2.0, waves_per_row: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """blend_device for lists the caller brings: numpy (ids[B, keep], value, source, count[B]) for `a_ids` [B, ka] /
        `a_scores` and `b_ids` [B, kb] / `b_scores` (a position with -1, an id outside the catalogue or a non-finite score ends its
        list); counts default to the widths.  `row_ids` given: B is weighted by the contacts of those rows of the resident X
        (a row outside the matrix has none), with the counts of `contact_counts` (a CSR of integers over X's rows, or None)
        where it stores one; otherwise by `weight_b`."""
        lists = [self._host_lists(a_ids, a_scores, a_counts), self._host_lists(b_ids, b_scores, b_counts)]
        if lists[0][0].shape[0] != lists[1][0].shape[0]:
            raise ValueError("both lists must have one row per row")
        contacts = row_ids is not None
        d_rows = cn = None
        if contacts:
            if not self._X:
                raise RuntimeError("set_interactions() must be called before blend with contacts")
            rows = np.asarray(row_ids, dtype=np.int64)
            if rows.shape != (lists[0][0].shape[0],):
                raise ValueError("row_ids must hold one entry per row")
            d_rows = self._up(self._rows32(rows, self.n_users))
            if contact_counts is not None:
                C = sp.csr_matrix(contact_counts)
                if C.shape[0] != self.n_users:
                    raise ValueError(f"contact_counts must have one row per row of X ({self.n_users}), got {C.shape[0]}")
                C.sort_indices()
                cn = (self._up(C.indptr.astype(np.int32)), self._up(C.indices.astype(np.int32)),
                      self._up(np.clip(C.data, -2 ** 31, 2 ** 31 - 1).astype(np.int32)))
        dev = [tuple(self._up(a) for a in lst) for lst in lists]
        out = self.blend_device(*dev[0], *dev[1], keep, weight_b, contacts, k, mnz, d_rows=d_rows, cn=cn, waves_per_row=waves_per_row)
        return tuple(t.cpu().numpy() for t in out)

    # ------------------------------------------------------------------------------ factor scorer (dense vectors, top-k per row)
    FACTOR_MAX_DIM = 256        # dim / top_k limits of rtrec_factor_topk
    FACTOR_MAX_K = 128

    @staticmethod
    def _as_float32(a, what: str) -> np.ndarray:
        """`a` as a float32 array; a value that is no float32 number is refused (scores are float32 fmaf chains of what is stored)."""
        a = np.asarray(a)
        a32 = np.ascontiguousarray(a, dtype=np.float32)
        if a.dtype != np.float32 and not np.array_equal(a32.astype(a.dtype), a, equal_nan=True):
            raise ValueError(f"{what} holds values that are not float32 numbers: factor scores are float32 sums of the stored "
                             "vectors, convert them first (and accept what that does to the ranking)")
        return a32

    def set_factors(self, user_vectors, item_vectors, user_index: Optional[np.ndarray] = None,
                    item_mask: Optional[np.ndarray] = None) -> None:
        """Upload the vectors of a factor model somebody else trained: `user_vectors` [n_p, dim] and `item_vectors`
        [n_items, dim] (stored transposed, component-major, so that neighbouring items are one contiguous read); `user_index`
        [n_users] int names the vector of every row of X (-1: none; None: row x has vector x, rows beyond n_p none);
        `item_mask` [n_items] marks the items that may be listed at all (None: all).  Biases are components the caller stacks
        (utils/factors.stack_bias).  The shapes are checked against the resident X and W; with several ranks every rank keeps
        all vectors and answers for the rows it is asked about."""
        P = self._as_float32(user_vectors, "user_vectors")
        Q = self._as_float32(item_vectors, "item_vectors")
        if P.ndim != 2 or Q.ndim != 2 or P.shape[1] != Q.shape[1]:
            raise ValueError(f"user and item vectors must be two matrices of one width, got {P.shape} and {Q.shape}")
        dim = int(P.shape[1])
        if not 1 <= dim <= self.FACTOR_MAX_DIM:
            raise ValueError(f"factor vectors of 1..{self.FACTOR_MAX_DIM} components are supported, got {dim}")
        n_items = int(self._W["n_items"]) if self._W else (self.n_items if self._X else int(Q.shape[0]))
        if int(Q.shape[0]) != n_items:
            raise ValueError(f"item_vectors must have one row per item of the catalogue ({n_items}), got {Q.shape[0]}")
        d_index = None
        if user_index is not None:
            idx = np.asarray(user_index, dtype=np.int64)
            if not self._X or idx.shape != (self.n_users,):
                raise ValueError(f"user_index must hold one entry per row of the resident X, got {idx.shape}")
            d_index = self.be.to_dev(np.where((idx >= 0) & (idx < P.shape[0]), idx, -1).astype(np.int32))
        d_mask = None
        if item_mask is not None:
            d_mask = self._upload_item_mask(item_mask, n_items)
        self._F = {"p": self.be.to_dev(P), "qt": self.be.to_dev(np.ascontiguousarray(Q.T)), "index": d_index, "mask": d_mask,
                   "dim": dim, "n_p": int(P.shape[0]), "n_items": n_items}
        self._take_item_norms(0)

    def _upload_item_mask(self, item_mask, n_items: int):
        m = np.asarray(item_mask)
        if m.shape != (n_items,):
            raise ValueError(f"item_mask must hold one entry per item ({n_items}), got {m.shape}")
        return self.be.to_dev((m != 0).astype(np.uint8))

    @staticmethod
    def _feature_csr(features, n_cols: int, what: str) -> sp.csr_matrix:
        """`features` as a float32 CSR over `n_cols` table rows, its entries in the order they are stored (the kernel adds them
        in that order: nothing is sorted or merged here)."""
        F = features if sp.isspmatrix_csr(features) else sp.csr_matrix(features)
        if F.shape[1] != n_cols:
            raise ValueError(f"{what} must have one column per row of its table ({n_cols}), got {F.shape[1]}")
        if F.nnz >= 2 ** 31:
            raise ValueError(f"{what} stores {F.nnz} entries; offsets are int32")
        if F.dtype != np.float32:
            F = sp.csr_matrix((SlimEngine._as_float32(F.data, what), F.indices, F.indptr), shape=F.shape)
        return F

    def _upload_feature_csr(self, F: sp.csr_matrix):
        """(ptr, col, val or None) device tensors of a feature CSR; all-ones values are not uploaded (d_f_val == NULL)."""
        val = None if (F.data == 1.0).all() else self._up(np.ascontiguousarray(F.data, dtype=np.float32))
        return self._up(F.indptr.astype(np.int32)), self._up(F.indices.astype(np.int32)), val

    def _feature_table(self, table, bias, what: str) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        E = self._as_float32(table, f"{what}_table")
        if E.ndim != 2:
            raise ValueError(f"{what}_table must be a matrix [features, components], got {E.shape}")
        b = None
        if bias is not None:
            b = self._as_float32(bias, f"{what}_bias").reshape(-1)
            if b.shape[0] != E.shape[0]:
                raise ValueError(f"{what}_bias must hold one entry per row of {what}_table ({E.shape[0]}), got {b.shape[0]}")
        return E, b

    def set_feature_factors(self, user_features, user_table, item_features, item_table, user_bias=None, item_bias=None) -> None:
        """The vectors of a factor model with feature rows, computed on the device: `user_features` is a scipy CSR with one row
        per row of the resident X and one column per row of `user_table` [user features, dim_e] (float32 numbers: LightFM's
        user_embeddings), `item_features` / `item_table` the same over the items of W; `user_bias` / `item_bias` [features]
        go in on both sides or on neither and are stacked as the reference stacks them ([b, 1, e...] . [1, b, e...]).  An
        entity's vector is its feature row times the table, entry by entry in storage order with a separately rounded
        multiply and add (csrc/feature_repr.hip; the comment of rtrec_feature_repr in include/rtrec_amd_ext.h), written
        straight into the matrices factor_topk reads -- the item matrix component-major, no host transpose.  A row without
        an entry in range has no vector (users) or is never listed (items).  The tables stay on the device for
        feature_vectors_device().  Leaves the engine as set_factors() leaves it."""
        from ._native import FEATURE_ITEM, FEATURE_PLAIN, FEATURE_USER
        be, torch = self.be, self.be.torch
        if (user_bias is None) != (item_bias is None):
            raise ValueError("biases go in on both sides or on neither: the stacked slots pair a bias with a constant 1")
        Eu, bu = self._feature_table(user_table, user_bias, "user")
        Ei, bi = self._feature_table(item_table, item_bias, "item")
        if Eu.shape[1] != Ei.shape[1]:
            raise ValueError(f"user_table and item_table must have one width, got {Eu.shape} and {Ei.shape}")
        dim_e = int(Eu.shape[1])
        dim = dim_e + (2 if bu is not None else 0)
        if dim_e < 1 or dim > self.FACTOR_MAX_DIM:
            raise ValueError(f"factor vectors of 1..{self.FACTOR_MAX_DIM} components are supported (the two bias slots included), got {dim}")
        if not self._X:
            raise RuntimeError("set_interactions() must be called before set_feature_factors")
        n_users = self.n_users
        n_items = int(self._W["n_items"]) if self._W else self.n_items
        Fu = self._feature_csr(user_features, Eu.shape[0], "user_features")
        Fi = self._feature_csr(item_features, Ei.shape[0], "item_features")
        if Fu.shape[0] != n_users:
            raise ValueError(f"user_features must have one row per row of the resident X ({n_users}), got {Fu.shape[0]}")
        if Fi.shape[0] != n_items:
            raise ValueError(f"item_features must have one row per item of the catalogue ({n_items}), got {Fi.shape[0]}")
        sides = {"user": {"e": be.to_dev(Eu), "bias": None if bu is None else be.to_dev(bu), "dim_e": dim_e,
                          "layout": FEATURE_PLAIN if bu is None else FEATURE_USER},
                 "item": {"e": be.to_dev(Ei), "bias": None if bi is None else be.to_dev(bi), "dim_e": dim_e,
                          "layout": FEATURE_PLAIN if bi is None else FEATURE_ITEM}}
        p = be.empty((n_users, dim), torch.float32)
        p_has = be.empty((n_users,), torch.uint8)
        qt = be.empty((dim, n_items), torch.float32)
        q_has = be.empty((n_items,), torch.uint8)
        if n_users:
            be.feature_repr(None, self._upload_feature_csr(Fu), sides["user"]["e"], dim_e, sides["user"]["bias"], sides["user"]["layout"],
                            n_users, p, dim, 1, p_has)
        if n_items:
            be.feature_repr(None, self._upload_feature_csr(Fi), sides["item"]["e"], dim_e, sides["item"]["bias"], sides["item"]["layout"],
                            n_items, qt, 1, n_items, q_has)
        rows = torch.arange(n_users, dtype=torch.int32, device=p.device)
        index = torch.where(p_has != 0, rows, torch.full_like(rows, -1))
        self._F = {"p": p, "qt": qt, "index": index, "mask": q_has, "dim": dim, "n_p": n_users, "n_items": n_items, "tables": sides}
        self._take_item_norms(1 if bi is not None else 0)       # (the reference's target matrix: [b, e...] of [1, b, e...])

    def feature_vectors_device(self, features_csr, side: str = "user"):
        """(vectors[n, dim] float32, has[n] uint8) device tensors for ad-hoc feature rows -- request-time tags, cold users --
        against the table set_feature_factors() kept for `side` ("user" or "item"): the same chain, the same stacking."""
        be, torch = self.be, self.be.torch
        tables = self._F.get("tables") if self.has_factors() else None
        if tables is None:
            raise RuntimeError("set_feature_factors() must be called before feature_vectors_device")
        if side not in tables:
            raise ValueError(f"side must be 'user' or 'item', got {side!r}")
        T = tables[side]
        F = self._feature_csr(features_csr, int(T["e"].shape[0]), "features_csr")
        n, dim = int(F.shape[0]), int(self._F["dim"])
        vec = be.empty((n, dim), torch.float32)
        has = be.empty((n,), torch.uint8)
        if n:
            be.feature_repr(None, self._upload_feature_csr(F), T["e"], T["dim_e"], T["bias"], T["layout"], n, vec, dim, 1, has)
        return vec, has

    def clear_factors(self) -> None:
        self._F = {}
        self._als = None

    def has_factors(self) -> bool:
        return bool(getattr(self, "_F", None))

    def _factor_topk_brought(self, rows: np.ndarray, vectors, vector_has, mask, filter_interacted: bool, top_k: int,
                             item_splits: int, ids, scores, count) -> None:
        """The jobs of factor_topk_device that bring their own vectors (`vectors` [n_rows, >= dim], `vector_has` [n_rows] uint8
        or None).  A job whose row lies outside X is a cold user: its vector is scored over the catalogue with nothing
        filtered (the op with row_ids = NULL and the brought matrix as `p`).  A job with a row of X -- request-time tags of a
        known user -- is scored against that row: a temporary index over X's rows points into the brought matrix, and since
        an index names one vector per row, a batch that names a row twice is split into rounds in which each row occurs once."""
        be, torch = self.be, self.be.torch
        F = self._F
        dev = vectors.device
        n_users = self.n_users

        def run(pos: np.ndarray, warm: bool) -> None:
            whole = len(pos) == len(rows)
            d_pos = None if whole else be.to_dev(pos.astype(np.int64))
            p = vectors if whole else vectors.index_select(0, d_pos)
            local = torch.arange(len(pos), dtype=torch.int32, device=dev)
            if vector_has is not None:
                h = vector_has if whole else vector_has.index_select(0, d_pos)
                local = torch.where(h != 0, local, torch.full_like(local, -1))
            o_ids, o_sc = (ids, scores) if whole else (be.empty((len(pos), top_k), torch.int32), be.empty((len(pos), top_k), torch.float32))
            o_cnt = count if whole else be.zeros((len(pos),), torch.int32)
            if warm:
                d_x = be.to_dev(rows[pos].astype(np.int64))
                index = torch.full((n_users,), -1, dtype=torch.int32, device=dev)
                index[d_x] = local
                be.factor_topk(d_x.to(torch.int32), index, n_users, p, F["qt"], F["n_items"], F["dim"], mask,
                               self._x_csr() if filter_interacted else None, bool(filter_interacted), top_k, o_ids, o_sc, o_cnt,
                               item_splits=item_splits)
            else:
                be.factor_topk(None, local if vector_has is not None else None, len(pos), p, F["qt"], F["n_items"], F["dim"], mask,
                               None, False, top_k, o_ids, o_sc, o_cnt, item_splits=item_splits)
            if not whole:
                ids[d_pos], scores[d_pos], count[d_pos] = o_ids, o_sc, o_cnt

        in_x = (rows >= 0) & (rows < n_users)
        if (~in_x).any():
            run(np.flatnonzero(~in_x), False)
        if in_x.any():
            pos = np.flatnonzero(in_x)
            order = np.argsort(rows[pos], kind="stable")
            srt = rows[pos][order]
            first = np.r_[0, np.flatnonzero(np.diff(srt)) + 1]
            occ = np.empty(len(pos), dtype=np.int64)          # the how-manieth job of its row
            occ[order] = np.arange(len(pos)) - np.repeat(first, np.diff(np.r_[first, len(pos)]))
            for k in range(int(occ.max()) + 1):
                run(pos[occ == k], True)

    def _factor_scan_front(self, name: str, n_rows: int, top_k: int, item_splits: int, item_mask):
        """The common front of factor_topk_device and similar_factor_device: the ranges of top_k and item_splits, the resident
        mask merged with `item_mask`, and the outputs: (mask, ids[n_rows, top_k], scores[same], count[n_rows])."""
        be, torch, F = self.be, self.be.torch, self._F
        if not 1 <= top_k <= self.FACTOR_MAX_K:
            raise ValueError(f"{name}: top_k must lie in 1..{self.FACTOR_MAX_K}, got {top_k}")
        if not 0 <= int(item_splits) <= 64:
            raise ValueError(f"{name}: item_splits must lie in 0..64, got {item_splits}")
        mask = F["mask"]
        if item_mask is not None:
            if int(item_mask.numel()) != F["n_items"]:
                raise ValueError(f"item_mask must hold one entry per item ({F['n_items']})")
            mask = item_mask if mask is None else (item_mask.to(torch.uint8) * mask)
        return (mask, be.empty((n_rows, top_k), torch.int32), be.empty((n_rows, top_k), torch.float32),
                be.zeros((n_rows,), torch.int32))

    def factor_topk_device(self, d_rows, n_rows: int, top_k: int, filter_interacted: bool = True, item_mask=None,
                           item_splits: int = 0, vectors=None, vector_has=None):
        """Device tensors (ids[n_rows, top_k] int32, scores[n_rows, top_k] float32, count[n_rows] int32): per row `d_rows[r]`
        of the resident X (int32 device tensor; None = rows 0 .. n_rows-1) the best top_k items by the dot product of the
        row's vector with the item vectors -- a float32 fmaf chain over ascending components -- among the items the resident
        mask and `item_mask` (a uint8 device tensor over the items, or None) admit and, with `filter_interacted`, the row does
        not store; the larger score first, the lower id among equal ones; -1 / -inf behind count.  A row without a vector, or
        outside X, gets an empty list.  The contract is the comment of rtrec_factor_topk in include/rtrec_amd_ext.h.
        `item_splits`: catalogue chunks per row block, 0 = the library's choice; the answer never depends on it.
        `vectors` [n_rows, dim] (a float32 device tensor, e.g. from feature_vectors_device) makes every job bring its own
        vector instead of the resident one of its row, `vector_has` [n_rows] uint8 says which jobs have one (None: all): a
        job with a row of X is scored against that row as usual, a job WITHOUT one (row < 0 or beyond X: a cold user) is
        scored over the catalogue with nothing filtered.  `d_rows` may then be a host array (it is read on the host)."""
        be, torch = self.be, self.be.torch
        if not self.has_factors():
            raise RuntimeError("set_factors() must be called before factor_topk")
        if not self._X:
            raise RuntimeError("set_interactions() must be called before factor_topk")
        F = self._F
        top_k, n_rows = int(top_k), int(n_rows)
        mask, ids, scores, count = self._factor_scan_front("factor_topk", n_rows, top_k, item_splits, item_mask)
        if self._W and F["n_items"] != int(self._W["n_items"]):
            raise ValueError(f"the resident factors cover {F['n_items']} items, W has {self._W['n_items']}: call set_factors() again")
        if F["index"] is not None and int(F["index"].numel()) != self.n_users:
            raise ValueError(f"the resident user_index covers {int(F['index'].numel())} rows, X has {self.n_users}: call set_factors() again")
        if n_rows == 0:
            return ids, scores, count
        if vectors is not None:
            if vectors.dim() != 2 or int(vectors.shape[0]) != n_rows or int(vectors.shape[1]) < F["dim"] or vectors.dtype != torch.float32:
                raise ValueError(f"vectors must be a float32 tensor [n_rows = {n_rows}, >= dim = {F['dim']}], got {tuple(vectors.shape)}")
            if vector_has is not None and int(vector_has.numel()) != n_rows:
                raise ValueError(f"vector_has must hold one entry per job ({n_rows})")
            rows = (np.arange(n_rows) if d_rows is None else
                    np.asarray(d_rows.cpu().numpy() if hasattr(d_rows, "cpu") else d_rows)).astype(np.int64).reshape(-1)
            if len(rows) != n_rows:
                raise ValueError(f"d_rows must hold one entry per job ({n_rows})")
            self._factor_topk_brought(rows, vectors.contiguous(), vector_has, mask, bool(filter_interacted), top_k, int(item_splits),
                                      ids, scores, count)
            return ids, scores, count
        be.factor_topk(d_rows, F["index"], self.n_users, F["p"], F["qt"], F["n_items"], F["dim"], mask,
                       self._x_csr() if filter_interacted else None, bool(filter_interacted), top_k, ids, scores, count,
                       item_splits=int(item_splits))
        return ids, scores, count

    def factor_topk_rows(self, row_ids: Sequence[int], top_k: int = 10, filter_interacted: bool = True,
                         item_mask: Optional[np.ndarray] = None, item_splits: int = 0, vectors=None, vector_has=None
                         ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """factor_topk_device for host row ids (a row outside X gets an empty list -- or, with brought `vectors`, is a cold
        user): numpy (ids[B, top_k], scores, count[B])."""
        rows = np.asarray(row_ids, dtype=np.int64).reshape(-1)
        rows = np.where((rows >= 0) & (rows < self.n_users), rows, -1).astype(np.int32)
        d_rows = rows if vectors is not None else self._up(rows)
        d_mask = None if item_mask is None else self._upload_item_mask(item_mask, self._F["n_items"] if self._F else self.n_items)
        out = self.factor_topk_device(d_rows, len(rows), top_k, filter_interacted, d_mask, item_splits, vectors=vectors,
                                      vector_has=vector_has)
        return tuple(t.cpu().numpy() for t in out)

    # ------------------------------------------------------------------------------ training the factor scorer (implicit ALS)
    ALS_MAX_DIM = 64            # dim limit of rtrec_factor_gram / rtrec_factor_als_solve (solver="cholesky")
    ALS_CG_MAX_DIM = 256        # dim limit of rtrec_factor_gram_wide / rtrec_factor_als_cg (solver="cg"): what the scorer serves
    ALS_CG_MAX_STEPS = 64       # cg_steps limit of rtrec_factor_als_cg
    ALS_SOLVERS = ("cholesky", "cg")

    @classmethod
    def als_solver_check(cls, dim: int, solver: str, cg_steps: int) -> None:
        """ValueError unless `solver` is known, `dim` lies within its limit and, for "cg", `cg_steps` in 1..64."""
        if solver not in cls.ALS_SOLVERS:
            raise ValueError(f"solver must be one of {cls.ALS_SOLVERS}, got {solver!r}")
        if solver == "cholesky":
            if not 1 <= dim <= cls.ALS_MAX_DIM:
                raise ValueError(f"factor vectors of 1..{cls.ALS_MAX_DIM} components can be trained, got {dim}")
            return
        if not 1 <= dim <= cls.ALS_CG_MAX_DIM:
            raise ValueError(f"factor vectors of 1..{cls.ALS_CG_MAX_DIM} components can be trained with solver='cg', got {dim}")
        if not 1 <= int(cg_steps) <= cls.ALS_CG_MAX_STEPS:
            raise ValueError(f"cg_steps must lie in 1..{cls.ALS_CG_MAX_STEPS}, got {cg_steps}")

    def _als_check(self, what: str) -> None:
        if not self._X:
            raise RuntimeError(f"set_interactions() must be called before {what}")
        if self.world_size > 1:
            raise ValueError(f"{what} trains on one rank: with several ranks train on one and bring the vectors with set_factors()")
        if self._W and getattr(self._W["dw"], "shard", None) is not None:
            raise ValueError(f"{what} needs the whole catalogue on this rank, and W is column-sharded (shard_w)")
        if not self.has_csc():
            raise RuntimeError(f"{what} reads both orientations of X: set_interactions(need_csc=True)")

    def _als_side(self, side: str):
        """(R as (ptr, idx, val), its number of rows, the matrix the side's half-step writes, the fixed one) of the training state."""
        if side not in ("user", "item"):
            raise ValueError(f"side must be 'user' or 'item', got {side!r}")
        X, T = self._X, self._als
        if side == "user":
            return (X["rptr"], X["rcol"], X["rval"]), self.n_users, T["P"], T["Q"]
        return (X["cptr"], X["crow"], X["cval"]), self.n_items, T["Q"], T["P"]

    def _als_order(self, side: str, ptr):
        """Every row of the side as an int32 job list, the longest row first (a row is one sequential chain on one wave: the
        long ones start first, as the scoring kernels do with d_row_order).  Kept beside X; the answer never depends on it."""
        torch = self.be.torch
        key = f"als_order_{side}"
        if key not in self._X:
            lens = (ptr[1:] - ptr[:-1]).to(torch.int64)
            self._X[key] = torch.argsort(lens, descending=True, stable=True).to(torch.int32)
        return self._X[key]

    def als_begin(self, dim: int, regularization: float, alpha: float, item_vectors, user_vectors=None, user_status=None,
                  item_status=None, *, solver: str = "cholesky", cg_steps: int = 3) -> None:
        """Open the training state: two row-major device matrices P [n_users, dim] and Q [rows of item_vectors, dim] (float32
        numbers), the regulariser and the confidence slope of the half-steps to come, and one status per row (1 = no vector
        yet).  fit_factors opens it with seeded item vectors alone; a caller that resumes from finished vectors brings both
        sides and their status.  `solver` names how the half-steps to come solve a row: "cholesky" (dim up to 64, exact) or
        "cg" (dim up to 256: `cg_steps` conjugate-gradient steps per row and half-step, warm-started from the row's vector)."""
        be, torch = self.be, self.be.torch
        self._als_check("als_begin")
        dim = int(dim)
        self.als_solver_check(dim, solver, cg_steps)
        reg, alpha = float(regularization), float(alpha)
        if not reg >= 0.0 or not alpha > 0.0:
            raise ValueError(f"regularization must be >= 0 and alpha > 0, got {regularization} and {alpha}")
        Q = self._as_float32(item_vectors, "item_vectors")
        if Q.ndim != 2 or Q.shape[1] != dim or Q.shape[0] > self.n_items:
            raise ValueError(f"item_vectors must be [<= {self.n_items} items, {dim}], got {Q.shape}")
        P = np.zeros((self.n_users, dim), np.float32)
        su = np.ones(self.n_users, np.uint8)
        if user_vectors is not None:
            Pu = self._as_float32(user_vectors, "user_vectors")
            if Pu.ndim != 2 or Pu.shape[1] != dim or Pu.shape[0] > self.n_users:
                raise ValueError(f"user_vectors must be [<= {self.n_users} rows of X, {dim}], got {Pu.shape}")
            P[:len(Pu)] = Pu
            su[:len(Pu)] = 0 if user_status is None else np.asarray(user_status, np.uint8)
        si = np.zeros(len(Q), np.uint8) if item_status is None else np.asarray(item_status, np.uint8)
        if si.shape != (len(Q),):
            raise ValueError(f"item_status must hold one entry per item vector ({len(Q)}), got {si.shape}")
        self._als = {"P": be.to_dev(P), "Q": be.to_dev(Q), "dim": dim, "reg": reg, "alpha": alpha,
                     "status": {"user": be.to_dev(su), "item": be.to_dev(si)}, "solver": solver, "cg_steps": int(cg_steps)}

    def als_half_step(self, side: str, rows: Optional[Sequence[int]] = None) -> Dict[int, int]:
        """One half-step of the open training state: the Gram matrix of the FIXED side (csrc/factor_gram.hip), then the solve
        of every row of `side` ("user": rows of X against the item vectors; "item": columns of X against the user vectors) or
        of the distinct rows named, written in place (csrc/factor_als.hip; the comments of rtrec_factor_gram and
        rtrec_factor_als_solve in include/rtrec_amd_ext.h are the contract).  Returns how many jobs ended with status 0
        (solved), 1 (a row outside the side, or without a usable entry: its vector is zero) and 2 (breakdown: zero too).
        With the state's solver "cg" the second call is rtrec_factor_als_cg (csrc/factor_als_cg.hip), warm-started from the
        vectors the state holds, and the Gram call is rtrec_factor_gram_wide above 64 components."""
        be, torch = self.be, self.be.torch
        self._als_check("als_half_step")
        T = getattr(self, "_als", None)
        if not T:
            raise RuntimeError("als_begin() or fit_factors() must be called before als_half_step")
        csr, n_rows, out, fixed = self._als_side(side)
        n_rows = min(n_rows, int(out.shape[0]))            # (an item X has gained since the vectors were made has none yet)
        dim = T["dim"]
        gram = be.empty((dim, dim), torch.float32)
        (be.factor_gram if dim <= self.ALS_MAX_DIM else be.factor_gram_wide)(fixed, int(fixed.shape[0]), dim, T["reg"], gram)
        if rows is None:
            jobs = self._als_order(side, csr[0])
            if int(jobs.numel()) != n_rows:
                jobs = jobs[jobs < n_rows]
        else:
            r = np.unique(np.asarray(rows, dtype=np.int64).reshape(-1))
            jobs = be.to_dev(r[(r >= 0) & (r < n_rows)].astype(np.int32))
        n_jobs = int(jobs.numel())
        status = be.zeros((n_jobs,), torch.uint8)
        if n_jobs:
            ptr = csr[0][:n_rows + 1].contiguous()
            if T.get("solver", "cholesky") == "cg":
                be.factor_als_cg(jobs, n_jobs, (ptr, csr[1], csr[2]), fixed, int(fixed.shape[0]), dim, gram, T["alpha"],
                                 T["cg_steps"], True, out, status)
            else:
                be.factor_als_solve(jobs, n_jobs, (ptr, csr[1], csr[2]), fixed, int(fixed.shape[0]), dim, gram, T["alpha"], out, status)
            T["status"][side][jobs.to(torch.int64)] = status
        counts = torch.bincount(status.to(torch.int64), minlength=3).cpu().numpy()
        return {s: int(counts[s]) for s in range(3)}

    def als_install(self) -> None:
        """Make the training state the resident factor model, exactly as set_factors() leaves one: P row-major, Q transposed on
        the device to component-major, user_index = -1 and item_mask = 0 where the last status is not 0, the item norms taken.
        Nothing visits the host."""
        be, torch = self.be, self.be.torch
        T = getattr(self, "_als", None)
        if not T:
            raise RuntimeError("als_begin() or fit_factors() must be called before als_install")
        n_items = int(self._W["n_items"]) if self._W else self.n_items
        Q, si = T["Q"], T["status"]["item"]
        if int(Q.shape[0]) != n_items:                      # the catalogue W covers and the trained items differ: cut or pad
            Qn = be.zeros((n_items, T["dim"]), torch.float32)
            sn = torch.ones((n_items,), dtype=torch.uint8, device=Q.device)
            k = min(n_items, int(Q.shape[0]))
            Qn[:k], sn[:k] = Q[:k], si[:k]
            Q, si = Qn, sn
        rows = torch.arange(self.n_users, dtype=torch.int32, device=Q.device)
        index = torch.where(T["status"]["user"] == 0, rows, torch.full_like(rows, -1))
        self._F = {"p": T["P"], "qt": Q.t().contiguous(), "index": index, "mask": (si == 0).to(torch.uint8), "dim": T["dim"],
                   "n_p": self.n_users, "n_items": n_items}
        self._take_item_norms(0)

    def fit_factors(self, dim: int = 32, iterations: int = 15, regularization: float = 0.01, alpha: float = 1.0,
                    seed: int = 0, *, solver: str = "cholesky", cg_steps: int = 3) -> Dict[str, Dict[int, int]]:
        """Train the factor scorer on the resident X by implicit-feedback ALS (Hu, Koren, Volinsky): `iterations` times a user
        half-step, then an item half-step.  Only the item matrix is initialised -- np.random.default_rng(seed)
        .standard_normal((n_items, dim)).astype(float32) * float32(0.01), made on the host and uploaded once -- and the result
        is installed as set_factors() would (als_install).  Deterministic: every operation of a half-step is pinned
        (include/rtrec_amd_ext.h).  `solver="cg"` runs `cg_steps` conjugate-gradient steps per row and half-step instead of
        the Cholesky solve, each warm-started from the last half-step's vector (the first user half-step from zero), and
        trains up to 256 components.  Returns the status counts of the last half-step of each side."""
        if int(iterations) < 1:
            raise ValueError(f"iterations must be at least 1, got {iterations}")
        self._als_check("fit_factors")
        self.als_solver_check(int(dim), solver, cg_steps)
        Q0 = np.random.default_rng(seed).standard_normal((self.n_items, int(dim))).astype(np.float32) * np.float32(0.01)
        self.als_begin(dim, regularization, alpha, Q0, solver=solver, cg_steps=cg_steps)
        counts = {}
        for _ in range(int(iterations)):
            counts["user"] = self.als_half_step("user")
            counts["item"] = self.als_half_step("item")
        self.als_install()
        return counts

    def als_vectors(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The training state on the host: (P, user status, Q, item status)."""
        T = self._als
        return (T["P"].cpu().numpy(), T["status"]["user"].cpu().numpy(), T["Q"].cpu().numpy(), T["status"]["item"].cpu().numpy())

    # ------------------------------------------------------------------------------ similar items from the factor vectors
    SIMILAR_BLEND_MAX_LIST = 1024       # ka / kb limit of rtrec_similar_blend

    def _take_item_norms(self, first_component: int) -> None:
        """The norms similar items will divide by, taken when the vectors are set or rebuilt.  A backend without factor_norms (a
        CPU stand-in that predates it) leaves them to the first call of item_norms_device."""
        if hasattr(self.be, "factor_norms"):
            self.item_norms_device(first_component)

    def item_norms_device(self, first_component: int = 0):
        """norms[n_items] float32 of the resident item vectors over the components first_component .. dim-1 (csrc/factor_norms.hip:
        the fmaf chain of the squares, a correctly rounded root).  set_factors / set_feature_factors take them for the first
        component the reference uses (0, or 1 for feature factors with biases); another first component is taken on first use.
        They are kept beside the vectors and dropped with them (a rebuild, clear_factors)."""
        if not self.has_factors():
            raise RuntimeError("set_factors() must be called before the item norms are taken")
        F, first = self._F, int(first_component)
        if not 0 <= first < F["dim"]:
            raise ValueError(f"first_component must lie in 0..{F['dim'] - 1}, got {first_component}")
        cache = F.setdefault("norms", {})
        if first not in cache:
            out = self.be.empty((F["n_items"],), self.be.torch.float32)
            if F["n_items"]:
                self.be.factor_norms(F["qt"][first:], F["n_items"], F["dim"] - first, 1, int(F["qt"].shape[1]), out)
            cache[first] = out
        return cache[first]

    def similar_factor_device(self, queries: Sequence[int], top_k: int = 10, first_component: int = 0, vectors=None,
                              write_cosine: bool = True, want_div: bool = False, item_mask=None, item_splits: int = 0):
        """Device tensors (ids[n, top_k] int32, scores[n, top_k] float32, count[n] int32, div[n] float32 or None): per query
        item (internal ids; one outside the catalogue has no vector) the top_k items by the cosine of the resident item
        vectors over the components first_component .. dim-1, the query and the items without a vector left out; the larger
        score first, the lower id among equal ones.  The ranking score is s1 = fl(dot / norm_i); with `write_cosine` the
        written score is fl(s1 / norm_q), otherwise s1 itself, and `want_div` returns the query norms for
        similar_blend.  `vectors` [n, dim] (a float32 device tensor of full-width vectors, e.g. feature_vectors_device(rows,
        "item")) makes every job bring its own query vector; its id then only names what is excluded (-1: nothing).  The
        contract is the comment of rtrec_factor_similar_topk in include/rtrec_amd_ext.h."""
        be, torch = self.be, self.be.torch
        if not self.has_factors():
            raise RuntimeError("set_factors() must be called before similar_factor")
        F = self._F
        top_k, first = int(top_k), int(first_component)
        q = np.asarray(queries, dtype=np.int64).reshape(-1)
        n, n_items, dim = len(q), F["n_items"], F["dim"] - first
        q = np.where((q >= 0) & (q < n_items), q, -1).astype(np.int32)
        mask, ids, scores, count = self._factor_scan_front("similar_factor", n, top_k, item_splits, item_mask)
        norms = self.item_norms_device(first)
        div = be.zeros((n,), torch.float32) if want_div else None
        if n == 0:
            return ids, scores, count, div
        p = p_norms = None
        if vectors is not None:
            if vectors.dim() != 2 or int(vectors.shape[0]) != n or int(vectors.shape[1]) < F["dim"] or vectors.dtype != torch.float32:
                raise ValueError(f"vectors must be a float32 tensor [n = {n}, >= dim = {F['dim']}], got {tuple(vectors.shape)}")
            p = vectors[:, first:F["dim"]].contiguous()
            p_norms = be.empty((n,), torch.float32)
            be.factor_norms(p, n, dim, dim, 1, p_norms)
        be.factor_similar_topk(self._up(q), p, p_norms, F["qt"][first:], n_items, dim, norms, mask, top_k, bool(write_cosine),
                               ids, scores, count, div=div, item_splits=int(item_splits))
        return ids, scores, count, div

    def similar_blend_device(self, a_ids, a_scores, a_counts, a_div, b_ids, b_scores, b_counts, exclude, keep: int,
                             n_items: Optional[int] = None, waves_per_row: int = 0):
        """Device tensors (ids[n, keep] int32, value[n, keep] FLOAT64, source[n, keep] int32, count[n] int32): list A (the
        factor side: s1 scores, divided here by `a_div[r]` after the cut) and list B (SLIM's) with `exclude[r]` taken out of
        both, each min-max normalised in float32 and summed per item id in float64, the larger value first, the earlier entry of
        the union among equal values.  `a_div` / `exclude` may be None.  The contract is the comment of rtrec_similar_blend in
        include/rtrec_amd_ext.h."""
        be, torch = self.be, self.be.torch
        if n_items is None:
            if not self._W:
                raise RuntimeError("Model must be fitted before calling similar_blend.")
            n_items = int(self._W["n_items"])
        n_rows, ka, kb, keep = int(a_ids.shape[0]), int(a_ids.shape[-1]), int(b_ids.shape[-1]), int(keep)
        if a_ids.dim() != 2 or b_ids.dim() != 2 or not 1 <= ka <= self.SIMILAR_BLEND_MAX_LIST or not 1 <= kb <= self.SIMILAR_BLEND_MAX_LIST:
            raise ValueError(f"similar_blend: two lists of 1..{self.SIMILAR_BLEND_MAX_LIST} items per row are supported, got {ka} and {kb}")
        if not 1 <= keep <= ka + kb:
            raise ValueError(f"similar_blend: keep must lie in 1..{ka + kb} (both list lengths together), got {keep}")
        if (tuple(a_scores.shape) != (n_rows, ka) or tuple(b_ids.shape) != (n_rows, kb) or tuple(b_scores.shape) != (n_rows, kb)
                or int(a_counts.numel()) != n_rows or int(b_counts.numel()) != n_rows):
            raise ValueError("similar_blend: scores must have the shape of their ids, both lists one row per row, counts one entry per row")
        ids = be.empty((n_rows, keep), torch.int32)
        value = be.empty((n_rows, keep), torch.float64)
        source = be.empty((n_rows, keep), torch.int32)
        count = be.zeros((n_rows,), torch.int32)
        if n_rows:
            be.similar_blend(n_items, a_ids.contiguous(), a_scores.contiguous(), a_counts.contiguous(), ka, a_div, b_ids.contiguous(),
                             b_scores.contiguous(), b_counts.contiguous(), kb, exclude, keep, ids, value, source, count,
                             waves_per_row=waves_per_row)
        return ids, value, source, count

    def similar_hybrid_device(self, queries: Sequence[int], top_k: int = 10, pool: Optional[int] = None, first_component: int = 0,
                              vectors=None, item_splits: int = 0):
        """The reference's hybrid similar_items in one device pass: the factor side's top-`pool` by s1 (similar_factor_device),
        W's column top-`pool` (similar_items_device) and the blend (similar_blend_device) hand their lists on in HBM; only
        (ids[n, keep], value[n, keep] float64, source, count[n]) with keep = min(top_k, 2 pool) are returned, as device
        tensors.  A query outside the catalogue has an empty SLIM side (and, without `vectors`, an empty factor side)."""
        be, torch = self.be, self.be.torch
        top_k = int(top_k)
        pool = top_k if pool is None else int(pool)
        if top_k < 1 or not 1 <= pool <= self.FACTOR_MAX_K:
            raise ValueError(f"similar_hybrid: top_k >= 1 and 1 <= pool <= {self.FACTOR_MAX_K} are supported, got {top_k} and {pool}")
        self._whole_w("similar_hybrid")
        n_items = int(self._W["n_items"])
        if self.has_factors() and self._F["n_items"] != n_items:
            raise ValueError(f"the resident factors cover {self._F['n_items']} items, W has {n_items}: call set_factors() again")
        q = np.asarray(queries, dtype=np.int64).reshape(-1)
        known = (q >= 0) & (q < n_items)
        q = np.where(known, q, -1).astype(np.int32)
        a_ids, a_sc, a_cnt, a_div = self.similar_factor_device(q, pool, first_component, vectors=vectors, write_cosine=False,
                                                               want_div=True, item_splits=item_splits)
        keep = min(top_k, 2 * pool)
        if len(q) == 0:
            return self.similar_blend_device(a_ids, a_sc, a_cnt, a_div, a_ids, a_sc, a_cnt, None, keep, n_items=n_items)
        b_ids, b_sc, b_cnt = self.similar_items_device(np.where(known, q, 0), pool)
        if not known.all():                                 # (W has no column for them: an empty list)
            b_cnt = torch.where(self._up(known.astype(np.uint8)) != 0, b_cnt, torch.zeros_like(b_cnt))
        return self.similar_blend_device(a_ids, a_sc, a_cnt, a_div, b_ids, b_sc, b_cnt, self._up(q), keep, n_items=n_items)

    # ------------------------------------------------------------------------------ catalogue ranks of held-out items
    RANKS_BLOCK_BYTES = 1 << 30     # the dense score block of one pass of catalogue_ranks_rows

    def _catalogue_layout(self) -> Optional[Dict[str, Any]]:
        """The plain tiled layout over ALL columns of W, whatever this rank's column block is.  With one rank, or with
        score_shard == "rows", that is _layout(compact=False); with several ranks and column shards every rank still holds the
        whole W (_whole_w has refused a column-sharded one) but its score layouts cover [col_lo, col_hi) only, so a layout over
        [0, n_items) is built for this call and cached beside the others.  None: W stores no weight."""
        W = self._W
        if W["col_lo"] == 0 and W["col_hi"] == W["n_items"]:
            return self._layout(compact=False)
        key = ("whole", self._tile_width(False, 10))
        if key not in W["layouts"]:
            dw: DeviceWeights = W["dw"]
            W["layouts"][key] = (build_tiled_w_device(self.be.torch, dw.rows, dw.cols, dw.vals, W["n_items"], 0, W["n_items"], key[1],
                                                      compact=False, dense_fill=None) if W["n_items"] > 0 else None)
        return W["layouts"][key]

    def catalogue_ranks_device(self, scores, d_rows, tg_ptr, tg_items, filter_interacted: bool, mode: int, xb=None):
        """Device tensors (above[n_tg] int32, tied[n_tg] int32, score[n_tg] float64, competing[n_rows] int32) for the targets
        `tg_ptr` [n_rows + 1] int64 / `tg_items` [n_tg] int32 of the dense score block `scores` [n_rows, >= W's n_items]
        (float32 or float64, e.g. what score_rows left: it never leaves HBM); `d_rows` names the row of `xb` = (ptr, col, val)
        device tensors (None: the resident X) each score row belongs to (None: row r).  The contract is the comment of
        rtrec_slim_catalogue_ranks in include/rtrec_amd_ext.h."""
        be, torch = self.be, self.be.torch
        dw = self._whole_w("catalogue_ranks")
        n_rows, n_tg = int(scores.shape[0]), int(tg_items.numel())
        above = be.empty((n_tg,), torch.int32)
        tied = be.empty((n_tg,), torch.int32)
        score = be.empty((n_tg,), torch.float64)
        competing = be.empty((n_rows,), torch.int32)
        if n_rows == 0:
            return above, tied, score, competing
        if xb is None:
            xb = self._x_csr()
        be.catalogue_ranks(dw.n_items, scores, d_rows, xb, bool(filter_interacted), int(mode), tg_ptr, tg_items, above, tied,
                           score, competing)
        return above, tied, score, competing

    def catalogue_ranks_rows(self, row_ids: Sequence[int], targets_ptr: np.ndarray, targets: np.ndarray,
                             filter_interacted: bool = True, mode: int = 0, block_bytes: Optional[int] = None
                             ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """At which position of the whole catalogue do the items `targets[targets_ptr[b] : targets_ptr[b + 1]]` stand for row
        `row_ids[b]` of the resident X: numpy (above[n_tg] int32, tied[n_tg] int32, score[n_tg] float64, competing[B] int32),
        the counts of rtrec_slim_catalogue_ranks (include/rtrec_amd_ext.h) over the score rows `recommend` ranks by.  Every
        rank that holds the whole W answers locally, over all columns (_catalogue_layout): there is no collective.  The
        rows are taken in passes whose dense score block [rows, n_items] (float64 when W accumulates in float64) stays within
        `block_bytes` (default RANKS_BLOCK_BYTES; one row at least): score_rows fills the block from the plain layout, the
        rank kernel reads it where it lies, and only the per-target and per-row results come back.  A row id outside the
        matrix is a user without a row: every score is 0.  `mode` is _native.TOPK_SPARSE or TOPK_DENSE."""
        be, torch = self.be, self.be.torch
        dw = self._whole_w("catalogue_ranks")
        if mode not in (_native.TOPK_SPARSE, _native.TOPK_DENSE):
            raise ValueError(f"catalogue_ranks: mode must be TOPK_SPARSE or TOPK_DENSE, got {mode}")
        row_ids = np.asarray(row_ids, dtype=np.int64)
        tptr = np.asarray(targets_ptr, dtype=np.int64)
        tgt = np.asarray(targets, dtype=np.int64)
        B, n_tg = len(row_ids), len(tgt)
        if tptr.shape != (B + 1,) or tptr[0] != 0 or tptr[-1] != n_tg or (np.diff(tptr) < 0).any():
            raise ValueError("catalogue_ranks: targets_ptr must hold len(row_ids) + 1 non-decreasing offsets from 0 to len(targets)")
        tgt32 = np.where((tgt >= 0) & (tgt < dw.n_items), tgt, -1).astype(np.int32)     # (an id beyond int32 is no column either)
        above, tied = np.full(n_tg, -1, np.int32), np.zeros(n_tg, np.int32)
        score, competing = np.full(n_tg, -np.inf, np.float64), np.zeros(B, np.int32)
        if B == 0:
            return above, tied, score, competing
        if not self._X:
            raise RuntimeError("set_interactions() must be called before catalogue_ranks_rows()")
        W = self._W
        f64 = bool(W["acc_f64"])
        dt = torch.float64 if f64 else torch.float32
        n_items = dw.n_items
        lay = self._catalogue_layout()
        row_bytes = max(n_items, 1) * (8 if f64 else 4)
        per_pass = int(max(1, min(B, (self.RANKS_BLOCK_BYTES if block_bytes is None else int(block_bytes)) // row_bytes)))
        rows32 = np.where((row_ids >= 0) & (row_ids < self.n_users), row_ids, -1).astype(np.int32)
        xb = self._x_csr()
        # The block is allocated zeroed once and reused by every pass without another memset: score_rows_kernel writes
        # out[row, c] for EVERY column c < n_cols of every row it is given (it zeroes its LDS tile, accumulates, then stores the
        # whole tile -- it never adds to what the buffer held), so nothing of the previous pass survives in the rows a pass
        # uses, and the rank kernel reads no other row.  The zeros only matter for a W without a layout (no stored weight at
        # all: no launch, every score 0), where they are never overwritten.
        block = be.zeros((per_pass, max(n_items, 1)), dt)
        for r0 in range(0, B, per_pass):
            r1 = min(B, r0 + per_pass)
            t0, t1 = int(tptr[r0]), int(tptr[r1])
            d_rows = self._up(rows32[r0:r1])
            sub = block[:r1 - r0]
            if lay is not None:
                be.score_rows(r1 - r0, d_rows, xb, W["n_items"], 0, lay, f64, sub)
            out = self.catalogue_ranks_device(sub, d_rows, self._up(tptr[r0:r1 + 1] - t0), self._up(tgt32[t0:t1]), filter_interacted,
                                              mode, xb)
            above[t0:t1], tied[t0:t1], score[t0:t1], competing[r0:r1] = (t.cpu().numpy() for t in out)
        return above, tied, score, competing

    # ------------------------------------------------------------------------------ audience of an item
    AUDIENCE_MAX_TOP_N = 1024   # top_n limit of rtrec_slim_audience_topk

    def _audience_check(self, top_n: int) -> DeviceWeights:
        """The one argument check of the audience calls: a W they can be scored from, and top_n within the kernel's range."""
        dw = self._whole_w("recommend_users")
        if not 1 <= int(top_n) <= self.AUDIENCE_MAX_TOP_N:
            raise ValueError(f"recommend_users: top_n in 1..{self.AUDIENCE_MAX_TOP_N} is supported, got {top_n}")
        return dw

    def has_csc(self) -> bool:
        """Whether the resident X carries its CSC orientation (set_interactions(need_csc=False) leaves it out)."""
        return "cptr" in self._X

    def _attach_csc(self, X_csc: sp.csc_matrix) -> None:
        """Add the CSC orientation of the resident X (the same matrix, sorted indices): the keys set_interactions(need_csc=True)
        would have left -- cptr / crow / cval and, because the fit reads them beside those, col_nnz and nonneg.  The CSR side
        is not touched, and the next set_interactions replaces the whole dict."""
        be = self.be
        if X_csc.shape != (self.n_users, self.n_items):
            raise ValueError(f"the CSC orientation is {X_csc.shape}, the resident X {(self.n_users, self.n_items)}")
        if not X_csc.has_sorted_indices:
            X_csc = X_csc.sorted_indices()
        X = self._X
        X["cptr"] = be.to_dev(np.asarray(X_csc.indptr, dtype=np.int32))
        X["crow"] = be.to_dev(np.asarray(X_csc.indices, dtype=np.int32))
        X["cval"] = be.to_dev(np.asarray(X_csc.data, dtype=np.float32))
        X["col_nnz"] = np.diff(np.asarray(X_csc.indptr, dtype=np.int64))
        X["nonneg"] = bool(X_csc.nnz == 0 or float(X_csc.data.min()) >= 0.0)

    def audience_device(self, d_items, n_q: int, top_n: int, filter_interacted: bool = True, d_user_mask=None):
        """Device tensors (users[n_q, top_n], scores[n_q, top_n], count[n_q], eligible[n_q]) for the query items `d_items`
        (int32 device tensor of internal item ids) against the resident X: the top_n users by score per item, the lower row
        first among equal scores, and the item's reach.  `d_user_mask`: int32 bitmap over the user rows (bit u & 31 of word
        u >> 5), None = everyone.  The contract is the comment of rtrec_slim_audience_topk in include/rtrec_amd.h.  The
        results stay in HBM.  Every rank that holds the whole W and X answers locally: there is no collective."""
        be, torch = self.be, self.be.torch
        dw = self._audience_check(top_n)
        top_n = int(top_n)
        if not self.has_csc():
            raise RuntimeError("set_interactions() with the CSC orientation must be called before audience_device()")
        users = be.empty((n_q, top_n), torch.int32)
        scores = be.empty((n_q, top_n), torch.float32)
        count = be.empty((n_q,), torch.int32)
        eligible = be.empty((n_q,), torch.int32)
        if n_q == 0:
            return users, scores, count, eligible
        X = self._X
        xptr, n_w = X["cptr"], dw.n_items          # the kernel reads the columns of X that W knows: X may have grown since the fit
        if xptr.numel() > n_w + 1:
            xptr = xptr[:n_w + 1]
        elif xptr.numel() < n_w + 1:
            xptr = torch.cat([xptr, xptr[-1:].expand(n_w + 1 - xptr.numel())])
        be.audience_topk(d_items, self.n_users, (xptr, X["crow"], X["cval"]), self._w_csc(), top_n, bool(filter_interacted), d_user_mask, users, scores, count, eligible)
        return users, scores, count, eligible

    def audience_items(self, item_ids: Sequence[int], top_n: int = 100, filter_interacted: bool = True,
                       candidate_rows: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """audience_device from the host: numpy (users[n_q, top_n], scores, count[n_q], eligible[n_q]) for the internal item
        ids `item_ids` (an id outside W: count 0).  `candidate_rows`: only these user rows are eligible (rows outside the
        matrix are ignored, an empty list leaves nobody); None = everyone."""
        be = self.be
        q = np.asarray(item_ids, dtype=np.int64).reshape(-1)
        top_n = int(top_n)
        if len(q) == 0:
            self._audience_check(top_n)
            return (np.empty((0, top_n), np.int32), np.empty((0, top_n), np.float32), np.empty(0, np.int32), np.empty(0, np.int32))
        q32 = np.where((q >= 0) & (q < 2 ** 31 - 1), q, -1).astype(np.int32)      # the kernel treats any id outside W as no column
        d_mask = None
        if candidate_rows is not None:
            rows = np.asarray(candidate_rows, dtype=np.int64).reshape(-1)
            rows = rows[(rows >= 0) & (rows < self.n_users)]
            bits = np.zeros(((self.n_users + 31) // 32) * 32, dtype=np.uint8)
            bits[rows] = 1
            d_mask = be.to_dev(np.packbits(bits, bitorder="little").view(np.int32))
        out = self.audience_device(self._up(q32), len(q32), top_n, filter_interacted, d_mask)
        return tuple(t.cpu().numpy() for t in out)


def coefficients_to_updates(targets: np.ndarray, items: np.ndarray, coef: np.ndarray, count: np.ndarray
                            ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Flatten fit_columns output to COO triples (row item i, column target j, value), explicit
    zeros included, ready for merge_coefficients()."""
    n, cap = items.shape
    mask = np.arange(cap)[None, :] < count[:, None]
    rows = items[mask].astype(np.int64)
    cols = np.repeat(targets.astype(np.int64), count)
    return rows, cols, coef[mask]


def merge_coefficients(W_old: Optional[sp.csc_matrix], n_items: int, rows: np.ndarray, cols: np.ndarray,
                       vals: np.ndarray, dtype=np.float32) -> sp.csc_matrix:
    """The LIL write-back of slim_elastic.py:271-274 / 371-374 / 554-557 as one vectorised merge:
    start from the old matrix (resized to n_items), then for every fitted (i, j): a non-zero value
    overwrites W[i, j], an explicit zero deletes it; entries of column j that the new solution does
    not mention survive."""
    if W_old is not None and W_old.nnz:
        Wo = W_old.tocoo()
        o_rows, o_cols, o_vals = Wo.row.astype(np.int64), Wo.col.astype(np.int64), Wo.data.astype(dtype)
        o_key = o_cols * n_items + o_rows
        n_key = cols * n_items + rows
        keep = ~np.isin(o_key, n_key)
        rows_all = np.concatenate([o_rows[keep], rows])
        cols_all = np.concatenate([o_cols[keep], cols])
        vals_all = np.concatenate([o_vals[keep], vals.astype(dtype)])
    else:
        rows_all, cols_all, vals_all = rows, cols, vals.astype(dtype)
    nz = vals_all != 0
    W = sp.csc_matrix((vals_all[nz], (rows_all[nz], cols_all[nz])), shape=(n_items, n_items), dtype=dtype)
    W.sort_indices()
    return W
