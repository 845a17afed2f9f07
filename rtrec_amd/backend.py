"""The device side of SlimEngine: W resident as sorted COO triples (DeviceWeights) and the thin marshalling layer over
librtrec_amd.so / torch.ops.rtrec_amd (HipBackend).  There is no CPU fallback: constructing a HipBackend without a GPU raises
NativeLibraryError.  (Split out of engine.py in round 4: VERDICT round 3, repo hygiene.)
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp

from . import _native
from . import settings
from .fit_plan import FitKnobs, FIT_MW_MAX_TARGETS  # noqa: F401  (the latter for importers of old)

XTY_SCRATCH_MAX_BYTES = 32 << 30   # a small fit call gets the one-pass X^T y (rtrec_fit_opts.d_xty_ws) while its scratch stays below this


class DeviceWeights:
    """W (I x I) resident on the device: COO triples sorted by (column, row) -- int64 rows / cols, float32 vals, no
    explicit zeros.  It is what a fit writes (SlimEngine.merge_fit), what the score layouts are built from
    (SlimEngine._layout) and what `item_similarity` is materialised from when the host asks for it (to_csc); `f64`
    records that the host-visible matrix is float64 (serial fit, slim_elastic.py:252), which selects the float64
    accumulator of the score kernels."""

    __slots__ = ("rows", "cols", "vals", "n_items", "f64", "lossy", "_host", "_csc", "shard")

    def __init__(self, rows, cols, vals, n_items: int, f64: bool, host: Optional[sp.csc_matrix] = None, lossy: bool = False):
        self.rows, self.cols, self.vals, self.n_items, self.f64 = rows, cols, vals, int(n_items), bool(f64)
        self.shard = None              # (rank, world): only this rank's column block of W is held (SlimEngine.shard_w)
        self.lossy = bool(lossy)       # uploaded from a float64 host matrix whose values are not float32 numbers
        self._host = host
        self._csc = None

    @property
    def nnz(self) -> int:
        return int(self.vals.numel())

    def csc_arrays(self, torch):
        """(ptr, row, val) int32 / int32 / float32 device tensors: the CSC view the item-to-item kernel reads."""
        if self._csc is None:
            ptr = torch.searchsorted(self.cols, torch.arange(self.n_items + 1, dtype=torch.int64, device=self.cols.device))
            self._csc = (ptr.to(torch.int32), self.rows.to(torch.int32), self.vals)
        return self._csc

    def to_csc(self, torch) -> sp.csc_matrix:
        """The host matrix (sorted indices), downloaded once."""
        if self._host is None:
            ptr, row, val = self.csc_arrays(torch)
            dt = np.float64 if self.f64 else np.float32
            self._host = sp.csc_matrix((val.cpu().numpy().astype(dt), row.cpu().numpy(), ptr.cpu().numpy()),
                                       shape=(self.n_items, self.n_items))
        return self._host


class HipBackend:
    """Thin marshalling layer over librtrec_amd.so; all arrays are torch CUDA tensors."""

    def __init__(self, device: Any = None):
        import torch
        if not torch.cuda.is_available():
            raise _native.NativeLibraryError("rtrec_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                                             "there is no CPU fallback")
        self.torch = torch
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.lib = _native.load()
        from . import ops as _ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
        self.ops = torch.ops.rtrec_amd
        self._xty_ws = None              # scratch of the one-pass X^T y of small fit calls (grown on demand)
        self._aux_stream = None
        # one-time costs of a process (custom-op dispatcher set-up, loading the gfx950 code objects)
        # belong here, next to the HIP context creation, not inside the first fit or recommend call
        w = torch.ones(1, dtype=torch.float32, device=self.device)
        self.ops.column_sqnorms(torch.tensor([0, 1], dtype=torch.int32, device=self.device), w, torch.empty_like(w))
        from .utils.device_store import DeviceInteractions
        DeviceInteractions(torch, self.device).warm_up(self.fold_pairs)
        k = torch.arange(4, dtype=torch.int64, device=self.device)         # the tensor ops of SlimEngine.merge_fit
        _ = (k // 2, k % 2, torch.isin(k, k[:2]), torch.argsort(k), k[k > 1], torch.cat([k, k]))

    # -- helpers -------------------------------------------------------------------------
    def to_dev(self, a: np.ndarray):
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.device, non_blocking=False)

    def to_dev_small(self, a: np.ndarray):
        """Upload of a request-sized array without a host-device round trip: staged in pinned memory (torch's caching host
        allocator keeps the block until the copy has run) and copied asynchronously on the current stream."""
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        if t.numel() > (1 << 16):
            return t.to(self.device, non_blocking=False)
        return t.pin_memory().to(self.device, non_blocking=True)

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device=self.device)

    def stream(self) -> C.c_void_p:
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def ptr(t) -> C.c_void_p:
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def synchronize(self):
        self.torch.cuda.synchronize(self.device)

    # -- one method per entry point, each a call of the matching torch.ops.rtrec_amd custom op
    #    (rtrec_amd/ops.py -> C-ABI); tests substitute a CPU stand-in with the same methods to
    #    exercise the multi-process orchestration without a GPU ---------------------------------
    def column_sqnorms(self, n_items, cptr, cval, out):
        self.ops.column_sqnorms(cptr, cval, out)

    def fit_workspace(self, n_users, n_items, slots, top_features):
        nbytes = int(self.lib.rtrec_slim_fit_workspace_bytes(n_users, n_items, slots, top_features))
        ws = self.empty((nbytes,), self.torch.uint8)
        self.ops.fit_workspace_init(ws, n_users, n_items, slots, top_features)
        return ws, self.zeros((1,), self.torch.int32)

    supports_gram = True
    supports_device_store = True     # X can stay resident as sorted COO (utils/device_store.py)
    fit_launch_options = True        # fit_columns takes fast / one_pass_xty / knobs (SlimEngine._launch_fit)

    def fit_columns(self, n_users, n_items, X, targets, cfg, out_items, out_coef, out_count, out_niter, cap,
                    ws, queue, slots, trace=None, gram=None, fast=0, one_pass_xty=False, knobs=FitKnobs()):
        """One launch of rtrec_slim_fit_columns_opt.  What to launch is the caller's decision (fit_plan.plan_fit: `fast`,
        `one_pass_xty`, and `knobs` for the tuning fields of rtrec_fit_opts); here only the scratch of the one-pass X^T y
        of all targets is sized, grown on demand, and given up where it would pass XTY_SCRATCH_MAX_BYTES."""
        g = gram or {}
        xty = None
        if one_pass_xty:
            need = int(self.lib.rtrec_slim_xty_workspace_bytes(n_users, n_items, int(X["rcol"].shape[0]), int(targets.shape[0])))
            if 0 < need <= XTY_SCRATCH_MAX_BYTES:
                if self._xty_ws is None or self._xty_ws.numel() < need:
                    self._xty_ws = None
                    self._xty_ws = self.empty((int(need * 1.25),), self.torch.uint8)
                xty = self._xty_ws
                if "col_order" not in X:          # longest columns first (lengths from the resident CSC pointer array)
                    X["col_order"] = self.torch.argsort(X["cptr"][1:] - X["cptr"][:-1], descending=True, stable=True).to(self.torch.int32)
        self.ops.fit_columns(X["cptr"], X["crow"], X["cval"], X["rptr"], X["rcol"], X["rval"], X["sqn"], targets,
                             n_users, n_items, float(cfg.l1_reg), float(cfg.l2_reg), float(cfg.tol), int(cfg.max_iter),
                             int(cfg.seed), bool(cfg.positive), int(cfg.top_features),
                             out_items, out_coef, out_count, out_niter, cap, ws, slots, queue, trace,
                             g.get("G"), g.get("index"), int(g.get("n", 0)), float(g.get("rel_err", 0.0)),
                             int(fast), knobs.kernel, knobs.colwalk_min_rows, knobs.screen_min, knobs.lane_max, xty,
                             X.get("col_order") if xty is not None else None, knobs.fold)

    def gram_matrix(self, X, n_users, n_items, n_top):
        """Gram matrix X_P^T X_P of the n_top most popular items in float64 for the fit kernel's Gram
        tracking (rtrec_slim_gram_matrix: densify + tiled float64 accumulation on the device)."""
        torch = self.torch
        col_nnz = X["col_nnz"]
        pop = np.argsort(-col_nnz, kind="stable")[:n_top]
        pop = pop[col_nnz[pop] > 0]
        P = int(len(pop))
        if P == 0:
            return None
        p64 = -(-P // 64) * 64
        gidx = np.full(n_items, -1, dtype=np.int32)
        gidx[pop] = np.arange(P, dtype=np.int32)
        d_gidx, d_top = self.to_dev(gidx), self.to_dev(pop.astype(np.int32))
        nbytes = int(self.lib.rtrec_slim_gram_workspace_bytes(n_users, P))
        ws = self.empty((nbytes,), torch.uint8)
        G = self.empty((p64, p64), torch.float64)
        self.ops.gram_matrix(X["cptr"], X["crow"], X["cval"], d_top, ws, G, n_users, n_items)
        return {"G": G, "index": d_gidx, "n": p64, "rel_err": max(1e-9, 64.0 * n_users * 2.0 ** -53), "items": pop}

    def score_workspace_bytes(self, n_rows, n_tiles, top_k):
        return int(self.lib.rtrec_slim_score_workspace_bytes(n_rows, n_tiles, top_k))

    supports_feature_rows = True
    supports_seg_layout = True

    def score_topk(self, n_rows, row_ids, xb, n_items, col_lo, lay, col_rank, top_k, filter_interacted, mode,
                   acc_f64, ids, sc, sc64, aux, cnt, ws, timer=0, diagnostics=0, use_fr=True, row_order=None, rescored=None, row_order_grouped=False,
                   use_sg=True, use_sg_heavy=True, flagged=None):
        fr = lay if (use_fr and lay.get("fr_w") is not None) else {}
        sg = lay.get("sg") or {} if (use_sg and not fr) else {}
        self.ops.score_topk(row_ids, xb[0], xb[1], xb[2], n_rows, n_items, lay["n_cols"], col_lo,
                            lay.get("col_ids"), lay.get("col_map"), int(lay.get("tile_cols", 0)), int(lay.get("n_tiles", 0)),
                            lay.get("tile_ptr"), lay.get("w_col"), lay.get("w_val"), lay.get("dense_idx"), lay.get("dense_val"),
                            lay.get("row_hdr"), col_rank, top_k, bool(filter_interacted), int(mode), bool(acc_f64),
                            ids, sc, sc64, aux, cnt, ws,
                            fr.get("fr_map"), fr.get("fr_col_ids"), fr.get("fr_col_map"), fr.get("fr_w"),
                            fr.get("fr_tile_rows"), fr.get("fr_tile_off"), fr.get("fr_super_kb"), fr.get("fr_super_tile"),
                            fr.get("fr_frag_tile"),
                            int(fr.get("fr_rows", 0)), int(fr.get("fr_tile_cols", 0)), int(fr.get("fr_n_tiles", 0)),
                            int(fr.get("fr_n_frags", 0)), int(fr.get("fr_n_super", 0)), int(fr.get("fr_buf_bytes", 0)),
                            fr.get("fr_scratch"),
                            row_order if (fr or sg) else None, int(timer), int(diagnostics), rescored,
                            # bit 1: the order is by descending length (the segment kernels rely on it: _row_order(allow_grouped=False))
                            int(bool(row_order_grouped)) | (int(bool(sg) and row_order is not None and not row_order_grouped) << 1),
                            sg.get("sg_info"), sg.get("sg_ptr"), sg.get("sg_ent"), sg.get("sg_bound"),
                            sg.get("sg_col_ids"), int(sg.get("sg_T", 0)), int(sg.get("sg_n_tiles", 0)), int(sg.get("sg_rows", 0)),
                            int(sg.get("sg_n_cols", 0)), sg.get("sg_trow_ptr"), sg.get("sg_trow"),
                            sg.get("sg_scratch") if use_sg_heavy else None, flagged,
                            self.aux_stream_handle() if (sg and use_sg_heavy and n_rows >= self.SG_FORK_MIN_ROWS) else 0)

    SG_FORK_MIN_ROWS = 8192          # = kSgForkMinRows (csrc/score_seg.hip.h)

    def aux_stream_handle(self) -> int:
        """A second stream of this backend (created on first use): the segment path's workgroup-per-long-user kernel runs on
        it beside the main kernel (rtrec_score_opts.aux_stream).  RTREC_AMD_SG_FORK=0 turns that off (A/B)."""
        if settings.raw("RTREC_AMD_SG_FORK", "1") == "0":
            return 0
        if self._aux_stream is None:
            self._aux_stream = self.torch.cuda.Stream(device=self.device)
        return int(self._aux_stream.cuda_stream)

    def decay_f32(self, raw, ts, rate: float, now: float):
        """float32(raw * rate ** ((now - ts) / 86400)) for resident arrays: rtrec_store_decay_device, plus the host's libm
        for the handful of entries the kernel flags as too close to a float32 rounding boundary (csrc/store_device.hip)."""
        torch = self.torch
        n = int(raw.shape[0])
        out = self.empty((n,), torch.float32)
        if n == 0:
            return out
        cap = max(1024, n >> 10)
        idx = self.empty((cap,), torch.int32)
        cnt = self.zeros((1,), torch.int32)
        self.ops.store_decay_device(raw, ts, float(rate), float(now), out, idx, cnt)
        k = int(cnt.item())
        sel = idx[:k].long() if k <= cap else torch.arange(n, device=raw.device)        # overflow: let the host do them all
        if sel.numel():
            v, t = raw[sel].cpu().numpy(), ts[sel].cpu().numpy()
            fix = np.empty(v.shape[0], np.float32)
            if self.lib.rtrec_store_decay(v.ctypes.data, t.ctypes.data, v.shape[0], float(rate), None, float(now), None,
                                          fix.ctypes.data, 0) != 0:
                raise _native.NativeLibraryError("rtrec_store_decay failed")
            out[sel] = torch.from_numpy(fix).to(out.device)
        return out

    def fold_pairs(self, order, start, delta, tstamp, old, lo: float, hi: float, upsert: bool):
        """(float64 values, float64 timestamps, float32 values) of a bulk batch's distinct pairs: rtrec_store_fold_device over
        the batch sorted by (user, item, arrival) -- see DeviceInteractions.ingest."""
        torch = self.torch
        g = int(start.shape[0]) - 1
        val, ts, v32 = self.empty((g,), torch.float64), self.empty((g,), torch.float64), self.empty((g,), torch.float32)
        self.ops.store_fold_device(order, start, delta, tstamp, old, float(lo), float(hi), bool(upsert), val, ts, v32)
        return val, ts, v32

    def timer_create(self) -> int:
        h = C.c_void_p()
        _native.check(self.lib.rtrec_timer_create(C.byref(h)), "rtrec_timer_create")
        return int(h.value)

    def timer_read(self, handle: int, reset: bool = False) -> Tuple[float, int]:
        ms, n = C.c_double(0), C.c_int64(0)
        _native.check(self.lib.rtrec_timer_read(C.c_void_p(handle), C.byref(ms), C.byref(n), int(reset)), "rtrec_timer_read")
        return float(ms.value), int(n.value)

    def timer_destroy(self, handle: int) -> None:
        self.lib.rtrec_timer_destroy(C.c_void_p(handle))

    def score_rows(self, n_rows, row_ids, xb, n_items, col_lo, lay, acc_f64, out):
        self.ops.score_rows(row_ids, xb[0], xb[1], xb[2], n_rows, n_items, lay["n_cols"], col_lo, lay["tile_cols"],
                            lay["n_tiles"], lay["tile_ptr"], lay["w_col"], lay["w_val"], bool(acc_f64), out)

    def merge_topk(self, n_rows, n_lists, top_k, g_ids, g_sc, g_sc64, g_aux, g_cnt, o_ids, o_sc, o_cnt):
        """g_* are [n_lists, n_rows, top_k] tensors (g_cnt [n_lists, n_rows]); they may be strided views
        into one packed all-gather buffer as long as the last dimension is contiguous."""
        self.ops.merge_topk(g_ids, g_sc, g_sc64, g_aux, g_cnt, top_k, o_ids, o_sc, o_cnt)

    def similar_topk(self, queries, W, top_k, ids, sc, cnt):
        self.ops.similar_topk(queries, W["cptr"], W["crow"], W["cval"], top_k, ids, sc, cnt)

    def explain_topk(self, row_ids, xb, n_items, W, ids, counts, list_k, top_m, items, contrib, support):
        """Per (row, list item): the top_m terms x_uj * w_ji of the score and their number (csrc/explain.hip); W as the CSC
        view of DeviceWeights.csc_arrays, ids [n_rows, >= list_k]."""
        self.ops.explain_topk(row_ids, xb[0], xb[1], xb[2], n_items, W["cptr"], W["crow"], W["cval"], ids, counts, list_k, top_m,
                              items, contrib, support)

    def score_pairs(self, row_ids, xb, n_items, W, ids, counts, list_k, top_k, filter_interacted, scores, support, order, count,
                    waves_per_row=0):
        """Per (row, list item): the score and its support, and per row the list positions by rank (csrc/score_pairs.hip); W as
        the CSC view of DeviceWeights.csc_arrays, ids [n_rows, >= list_k]; top_k == 0: order / count are empty tensors."""
        self.ops.score_pairs(row_ids, xb[0], xb[1], xb[2], n_items, W["cptr"], W["crow"], W["cval"], ids, counts, list_k, top_k,
                             bool(filter_interacted), int(waves_per_row), scores, support, order, count)

    def diversify_lists(self, n_items, W, ids, scores, counts, list_k, keep, lam, order, value, penalty, count, waves_per_row=0):
        """Per list: the greedy MMR order over W's similarities (csrc/diversify.hip; include/rtrec_amd_ext.h); W as the CSC view of
        DeviceWeights.csc_arrays, ids / scores [n_rows, >= list_k], the outputs [n_rows, keep] and [n_rows]."""
        self.ops.diversify_lists(W["cptr"], W["crow"], W["cval"], n_items, ids, scores, counts, list_k, keep, float(lam),
                                 int(waves_per_row), order, value, penalty, count)

    def list_quality(self, n_items, W, ids, counts, list_k, item_weight, exposure, n, sim_sum, linked, weight_sum, waves_per_row=0):
        """Per list: the counted positions, the intra-list similarity sum over W, its linked pairs and the sum of item_weight
        (csrc/list_quality.hip; include/rtrec_amd_ext.h); every counted position adds 1 to exposure.  W as the CSC view of
        DeviceWeights.csc_arrays, ids [n_rows, >= list_k], item_weight / exposure [n_items] or None, the outputs [n_rows]."""
        self.ops.list_quality(W["cptr"], W["crow"], W["cval"], n_items, ids, counts, list_k, item_weight, int(waves_per_row),
                              n, sim_sum, linked, weight_sum, exposure)

    def catalogue_ranks(self, n_items, scores, row_ids, xb, filter_interacted, mode, tg_ptr, tg_items, above, tied, score, competing):
        """Per target (row, item) of a dense score block: the competing columns above it and tied with it, its score, and per row
        the competing columns (csrc/catalogue_ranks.hip; include/rtrec_amd_ext.h).  scores [n_rows, >= n_items] float32 or
        float64, xb the (ptr, col, val) triple of X (val is not read), tg_ptr [n_rows + 1] int64 into tg_items int32."""
        self.ops.catalogue_ranks(scores, n_items, row_ids, xb[0], xb[1], bool(filter_interacted), int(mode), tg_ptr, tg_items,
                                 above, tied, score, competing)

    def blend_lists(self, n_items, a_ids, a_scores, a_counts, ka, b_ids, b_scores, b_counts, kb, keep, weight_b, contacts, k, mnz,
                    row_ids, xb, cn, out_ids, value, source, count, waves_per_row=0):
        """Per row: the union of list A and list B by item id, each min-max normalised, B weighted by `weight_b` or -- with
        `contacts` -- by how often the row's user touched the item, ranked by the summed value (csrc/blend.hip;
        include/rtrec_amd_ext.h).  a_* / b_* [n_rows, >= ka / kb] and [n_rows]; xb the (ptr, col, val) triple of X (val is not
        read) and cn the (ptr, col, val) int32 triple of the count CSR, each or both None; the outputs [n_rows, keep] and
        [n_rows]."""
        xb = (None, None) if xb is None else xb
        cn = (None, None, None) if cn is None else cn
        self.ops.blend_lists(n_items, a_ids, a_scores, a_counts, ka, b_ids, b_scores, b_counts, kb, keep, float(weight_b),
                             bool(contacts), float(k), bool(mnz), row_ids, xb[0], xb[1], cn[0], cn[1], cn[2], int(waves_per_row),
                             out_ids, value, source, count)

    FACTOR_AUTO_BLOCKS = 1024       # item_splits == 0: chunks until this many workgroups exist (the rule of csrc/factor_topk.hip)

    def factor_splits(self, n_rows, n_items, item_splits=0):
        """The number of catalogue chunks a factor_topk call of `n_rows` jobs runs with: `item_splits`, or for 0 the library's own
        rule (chunks until FACTOR_AUTO_BLOCKS workgroups of 32 jobs exist, at most 64), never more than the 32-item tiles."""
        blocks = max(1, (int(n_rows) + 31) // 32)
        s = int(item_splits) if item_splits else min(64, (self.FACTOR_AUTO_BLOCKS + blocks - 1) // blocks)
        return max(1, min(s, (int(n_items) + 31) // 32))

    def factor_workspace(self, n_rows, n_items, top_k, item_splits=0):
        """(splits, workspace) of a factor scan call: factor_splits' chunks and, for more than one, the uint8 tensor their partial
        lists live in (RTREC_FACTOR_TOPK_WORKSPACE_BYTES of include/rtrec_amd_ext.h), else None."""
        splits = self.factor_splits(n_rows, n_items, item_splits)
        return splits, (self.empty((int(n_rows) * splits * (int(top_k) * 8 + 4),), self.torch.uint8) if splits > 1 else None)

    def factor_topk(self, row_ids, p_index, n_x_rows, p, qt, n_items, dim, item_mask, xb, filter_interacted, top_k, ids, scores,
                    count, item_splits=0):
        """Per job: the top_k items by the fmaf chain of its vector (row p_index[x] of `p`, x = row_ids[r]) against the
        component-major item vectors `qt`, the mask and -- with `filter_interacted` -- the row of X = `xb` (ptr, col, val; val
        is not read) applied (csrc/factor_topk.hip; include/rtrec_amd_ext.h).  The partial lists of a chunked call live in
        factor_workspace's tensor."""
        splits, ws = self.factor_workspace(int(count.numel()), n_items, top_k, item_splits)
        xb = (None, None) if xb is None else xb
        self.ops.factor_topk(row_ids, p_index, int(n_x_rows), p, qt, int(n_items), int(dim), item_mask, xb[0], xb[1],
                             bool(filter_interacted), int(top_k), splits, ids, scores, count, ws)

    def feature_repr(self, job_rows, f_csr, table, dim_e, bias, layout, n_jobs, out, row_stride, comp_stride, has):
        """Per job: its sparse feature row (row job_rows[r] of `f_csr` = (ptr, col, val or None); job_rows None: row r) times the
        per-feature `table` [n_features, >= dim_e] -- an ordered, unfused float32 chain per slot -- stacked by `layout`
        (_native.FEATURE_PLAIN / FEATURE_USER / FEATURE_ITEM, the latter two with `bias` [n_features]) and written to
        out.flatten()[r * row_stride + c * comp_stride]; has [n_jobs] uint8 or None (csrc/feature_repr.hip;
        include/rtrec_amd_ext.h)."""
        self.ops.feature_repr(job_rows, f_csr[0], f_csr[1], f_csr[2], table, int(dim_e), bias, int(layout), int(n_jobs), out,
                              int(row_stride), int(comp_stride), has)

    def factor_norms(self, v, n, dim, row_stride, comp_stride, out):
        """Per vector: its Euclidean norm as the ordered fmaf chain of its squares and a correctly rounded root; component c of
        vector r is v.flatten()[r * row_stride + c * comp_stride] (csrc/factor_norms.hip; include/rtrec_amd_ext.h)."""
        self.ops.factor_norms(v, int(n), int(dim), int(row_stride), int(comp_stride), out)

    def factor_similar_topk(self, queries, p, p_norms, qt, n_items, dim, norms, item_mask, top_k, write_cosine, ids, scores, count,
                            div=None, item_splits=0):
        """Per query item: the top_k items by fl(dot / norm_i) against the component-major item vectors `qt`, the query and the
        masked items left out; the query's vector is column queries[r] of `qt`, or row r of `p` (with `p_norms`); `div` [n_rows]
        receives the query norms, `write_cosine` divides the written scores by them (csrc/factor_similar.hip;
        include/rtrec_amd_ext.h).  The workspace of a chunked call is factor_topk's."""
        splits, ws = self.factor_workspace(int(count.numel()), n_items, top_k, item_splits)
        self.ops.factor_similar_topk(queries, p, p_norms, qt, int(n_items), int(dim), norms, item_mask, int(top_k), splits,
                                     bool(write_cosine), ids, scores, count, div, ws)

    def similar_blend(self, n_items, a_ids, a_scores, a_counts, ka, a_div, b_ids, b_scores, b_counts, kb, exclude, keep, out_ids,
                      value, source, count, waves_per_row=0):
        """Per row: list A and list B cut, `exclude[r]` taken out, A divided by `a_div[r]`, each min-max normalised in float32,
        summed per item id in float64 (`value` is a float64 tensor), ranked (csrc/similar_blend.hip; include/rtrec_amd_ext.h)."""
        self.ops.similar_blend(int(n_items), a_ids, a_scores, a_counts, int(ka), a_div, b_ids, b_scores, b_counts, int(kb), exclude,
                               int(keep), int(waves_per_row), out_ids, value, source, count)

    GRAM_CHUNK = 1024        # rows of V per partial Gram: the contract constant of rtrec_factor_gram

    def factor_gram(self, v, n_v, dim, reg, gram):
        """gram[dim, dim] = V^T V + reg I of the row-major vectors `v` [>= n_v, >= dim]: fmaf chains per chunk of 1024 rows, the
        partials added in ascending order (csrc/factor_gram.hip; include/rtrec_amd_ext.h).  The partials live in a tensor of
        RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim) bytes."""
        chunks = (int(n_v) + self.GRAM_CHUNK - 1) // self.GRAM_CHUNK
        ws = self.empty((chunks * int(dim) * int(dim) * 4,), self.torch.uint8) if chunks else None
        self.ops.factor_gram(v, int(n_v), int(dim), float(reg), gram, ws)

    def factor_als_solve(self, job_rows, n_jobs, r_csr, v, n_v, dim, gram, alpha, out, status):
        """Per job: row job_rows[r] (None: row r) of R = `r_csr` (ptr, idx, val) solved against the fixed side `v` and its
        `gram`: the pinned build, Cholesky and substitutions of rtrec_factor_als_solve, the vector written in place into `out`
        [>= n_rows, >= dim], one uint8 `status` per job (csrc/factor_als.hip; include/rtrec_amd_ext.h)."""
        self.ops.factor_als_solve(job_rows, int(n_jobs), r_csr[0], r_csr[1], r_csr[2], v, int(n_v), int(dim), gram, float(alpha),
                                  out, status)

    def factor_gram_wide(self, v, n_v, dim, reg, gram):
        """factor_gram for vectors of up to 256 components: the same definition, one MFMA chain per (chunk, lower 32 x 32 tile)
        (csrc/factor_gram.hip, rtrec_factor_gram_wide; include/rtrec_amd_ext.h).  Equal to factor_gram bit for bit up to 64."""
        chunks = (int(n_v) + self.GRAM_CHUNK - 1) // self.GRAM_CHUNK
        ws = self.empty((chunks * int(dim) * int(dim) * 4,), self.torch.uint8) if chunks else None
        self.ops.factor_gram_wide(v, int(n_v), int(dim), float(reg), gram, ws)

    def factor_als_cg(self, job_rows, n_jobs, r_csr, v, n_v, dim, gram, alpha, cg_steps, warm_start, out, status, rs=None):
        """Per job: `cg_steps` pinned conjugate-gradient steps on the system factor_als_solve factors, started from the vector
        `out` holds (`warm_start`) or from zero, written in place; one uint8 `status` per job and, where `rs` is given, the last
        squared residual norm (csrc/factor_als_cg.hip, rtrec_factor_als_cg; include/rtrec_amd_ext.h).  dim up to 256."""
        self.ops.factor_als_cg(job_rows, int(n_jobs), r_csr[0], r_csr[1], r_csr[2], v, int(n_v), int(dim), gram, float(alpha),
                               int(cg_steps), bool(warm_start), out, status, rs)

    def audience_workspace_bytes(self, n_users, n_q, top_n):
        return int(self.lib.rtrec_slim_audience_workspace_bytes(n_users, n_q, top_n))

    def audience_topk(self, items, n_users, X, W, top_n, filter_interacted, user_mask, users, scores, count, eligible):
        """Per query item: the top_n users by score, their number and the item's reach (csrc/audience.hip); X = (cptr, crow, cval), its CSC
        orientation with as many columns as W, W as the CSC view of DeviceWeights.csc_arrays, user_mask an int32 bitmap or None."""
        ws = self.empty((max(self.audience_workspace_bytes(n_users, int(items.numel()), top_n), 8),), self.torch.uint8)
        self.ops.audience_topk(items, n_users, X[0], X[1], X[2], W["cptr"], W["crow"], W["cval"], top_n,
                               bool(filter_interacted), user_mask, users, scores, count, eligible, ws)
