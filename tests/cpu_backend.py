"""CPU stand-in for rtrec_amd.engine.HipBackend, built on the oracle.  TEST-ONLY.

Lets the multi-process orchestration of SlimEngine / SLIMElastic (column sharding, the
all-gather of per-shard top-k, the coefficient gather) run under gloo on a machine without a
GPU.  It is never importable from the product package; the product path has no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch

from oracle import slim_oracle as so


class OracleBackend:
    def __init__(self):
        self.torch = torch
        self.device = torch.device("cpu")

    def to_dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).copy())

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype)

    def synchronize(self):
        pass

    # ---- ops -------------------------------------------------------------------------
    def column_sqnorms(self, n_items, cptr, cval, out):
        out.zero_()

    def fit_workspace(self, n_users, n_items, slots, top_features):
        return torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)

    def fit_columns(self, n_users, n_items, X, targets, cfg, out_items, out_coef, out_count, out_niter, cap,
                    ws, queue, slots, trace=None, gram=None):
        Xc = sp.csc_matrix((X["cval"].numpy(), X["crow"].numpy(), X["cptr"].numpy()), shape=(n_users, n_items))
        tg = targets.numpy()
        L = so.lib()
        import ctypes as C
        for t, j in enumerate(tg):
            idx = np.empty(n_items, np.int32)
            val = np.empty(n_items, np.float32)
            nit, gap = C.c_int32(0), C.c_float(0)
            n = L.slim_oracle_fit_column(
                n_users, n_items, np.ascontiguousarray(Xc.data, np.float32), np.ascontiguousarray(Xc.indices, np.int32),
                np.ascontiguousarray(Xc.indptr, np.int32), int(j),
                # undo the scaling the engine applied: the oracle takes alpha / l1_ratio
                *self._alpha_l1(cfg, n_users), float(cfg.tol), int(cfg.max_iter), int(cfg.seed), int(cfg.positive),
                int(cfg.top_features), idx, val, C.byref(nit), C.byref(gap))
            out_items[t, :n] = torch.from_numpy(idx[:n])
            out_coef[t, :n] = torch.from_numpy(val[:n])
            out_count[t] = n
            out_niter[t] = nit.value

    @staticmethod
    def _alpha_l1(cfg, n_users):
        a, b = float(cfg.l1_reg) / n_users, float(cfg.l2_reg) / n_users   # alpha*l1, alpha*(1-l1)
        alpha = a + b
        return alpha, (a / alpha if alpha else 0.0)

    def _shard_w(self, n_items, col_lo, lay):
        # rebuild this shard's W (n_items x n_items, only the shard's columns populated)
        S, T = lay["tile_cols"], lay["n_tiles"]
        tp = lay["tile_ptr"].numpy().reshape(T, n_items + 1)
        wc = lay["w_col"].numpy().view(np.uint16).astype(np.int64)
        wv = lay["w_val"].numpy()
        rows, cols = [], []
        for t in range(T):
            cnt_t = np.diff(tp[t])
            rows.append(np.repeat(np.arange(n_items), cnt_t))
            loc = wc[tp[t, 0]:tp[t, -1]] + t * S
            cols.append(lay["col_ids"].numpy()[loc] if lay["col_ids"] is not None else loc + col_lo)
        vals = [wv]
        if lay.get("dense_idx") is not None:
            di = lay["dense_idx"].numpy().reshape(T, n_items)
            dv = lay["dense_val"].numpy().reshape(-1, S)
            for t, i in zip(*np.nonzero(di >= 0)):
                blk = dv[di[t, i]]
                nz = np.flatnonzero(blk)
                loc = nz + t * S
                rows.append(np.full(len(nz), i))
                cols.append(lay["col_ids"].numpy()[loc] if lay["col_ids"] is not None else loc + col_lo)
                vals.append(blk[nz])
        Wr = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n_items, n_items))
        return Wr

    def score_workspace_bytes(self, n_rows, n_tiles, top_k):
        return 1

    def score_topk(self, n_rows, row_ids, xb, n_items, col_lo, lay, col_rank, top_k, filter_interacted, mode,
                   acc_f64, ids, sc, sc64, aux, cnt, ws):
        Wr = self._shard_w(n_items, col_lo, lay)
        ptr, col, val = (t.numpy() for t in xb)
        Xall = sp.csr_matrix((val, col, ptr), shape=(len(ptr) - 1, n_items))
        rsel = row_ids.numpy() if row_ids is not None else np.arange(n_rows)
        if mode == 2:
            # candidate mode (slim_elastic.py:723-735): dense scores of the candidate columns, argsort()[-k:][::-1] with the
            # stable-argsort tie rule (DESIGN D1: later candidate first), zeros included, filter_interacted ignored
            cr = col_rank.numpy()
            cols = lay["col_ids"].numpy()[:lay["n_cols"]] if lay["col_ids"] is not None else np.arange(col_lo, col_lo + lay["n_cols"])
            cand = cols[cr[cols] >= 0]
            cand = cand[np.argsort(cr[cand], kind="stable")]
            dt = np.float64 if acc_f64 else np.float32
            S = (Xall[rsel].astype(dt) @ Wr.astype(dt).tocsc()[:, cand]).toarray()
            o_ids = np.full((n_rows, top_k), -1, np.int32)
            o_sc = np.full((n_rows, top_k), -np.inf, dt)
            o_aux = np.zeros((n_rows, top_k), np.int32)
            for r in range(n_rows):
                idx = np.argsort(S[r], kind="stable")[-top_k:][::-1] if len(cand) else np.empty(0, np.int64)
                o_ids[r, :len(idx)] = cand[idx]; o_sc[r, :len(idx)] = S[r, idx]; o_aux[r, :len(idx)] = cr[cand[idx]]
            ids.copy_(torch.from_numpy(o_ids)); sc.copy_(torch.from_numpy(o_sc.astype(np.float32)))
            cnt.fill_(min(top_k, len(cand)))
            aux.copy_(torch.from_numpy(o_aux))
            if sc64 is not None:
                sc64.copy_(torch.from_numpy(o_sc.astype(np.float64)))
            return
        Xsel = Xall[rsel]
        dt = np.float64 if acc_f64 else np.float32
        with np.errstate(all="ignore"):
            P = sp.csr_matrix(Xsel.astype(dt) @ Wr.astype(dt))     # scipy's csr_matmat: the product the reference ranks
        if np.isfinite(P.data).all():
            o_ids, o_sc, o_cnt = so.recommend_batch(Xsel, Wr, top_k=top_k, filter_interacted=filter_interacted,
                                                    dense=(mode == 1), use_f64=bool(acc_f64))
        else:
            # A score is NaN or infinite: the oracle's insertion order defines nothing once a NaN arrives.  The rule of
            # include/rtrec_amd.h on scipy's own product: NaN and -inf are never listed, +inf is a number.
            o_ids, o_sc, o_cnt = self._lists_of_product(P, Xsel, top_k, filter_interacted, mode == 1)
        ids.copy_(torch.from_numpy(o_ids)); sc.copy_(torch.from_numpy(o_sc)); cnt.copy_(torch.from_numpy(o_cnt))
        aux.zero_()
        if mode == 0:
            # the reference's tie key (csrc/score_first_touch.hip): position, in the user's row, of the first item whose row of
            # W stores a weight in the column -- lists of different column shards are merged by (score, key, id)
            Wc, Xs = Wr.tocsc(), Xall[rsel].tocsr()
            Wc.sort_indices(); Xs.sort_indices()
            o_aux = np.zeros((n_rows, top_k), np.int32)
            for r in range(n_rows):
                items = Xs.indices[Xs.indptr[r]:Xs.indptr[r + 1]]
                for k in range(int(o_cnt[r])):
                    rows_c = Wc.indices[Wc.indptr[o_ids[r, k]]:Wc.indptr[o_ids[r, k] + 1]]
                    pos = np.searchsorted(items, rows_c)
                    hit = (pos < len(items)) & (items[np.minimum(pos, max(len(items) - 1, 0))] == rows_c) if len(items) else np.zeros(len(rows_c), bool)
                    o_aux[r, k] = int(pos[hit].min()) if hit.any() else 0
            aux.copy_(torch.from_numpy(o_aux))
        if sc64 is not None:
            sc64.copy_(torch.from_numpy(o_sc.astype(np.float64)))

    @staticmethod
    def _lists_of_product(P, Xsel, top_k, filter_interacted, dense):
        """(ids, float32 scores, counts) from the rows of the product P = X W as scipy leaves them: a row's stored entries are
        its non-zero sums, LAST touched column first (csr_matmat's linked list) -- the list slim_elastic.py:782-818 sorts with
        a stable sorted(reverse=True).  DENSE (:744-779): every column, ties to the higher id."""
        B, n_cols = P.shape
        o_ids = np.full((B, top_k), -1, np.int32)
        o_sc = np.full((B, top_k), -np.inf, np.float32)
        o_cnt = np.zeros(B, np.int32)
        for r in range(B):
            cols, vals = P.indices[P.indptr[r]:P.indptr[r + 1]], P.data[P.indptr[r]:P.indptr[r + 1]]
            own = Xsel.indices[Xsel.indptr[r]:Xsel.indptr[r + 1]]
            if dense:
                sc = np.zeros(n_cols, P.dtype)
                sc[cols] = vals
                if filter_interacted:
                    sc[own] = -np.inf
                keep = np.flatnonzero(sc > -np.inf)                 # (NaN > -inf is false)
                order = keep[np.lexsort((-keep, -sc[keep]))][:top_k]
                sel, val = order, sc[order]
            else:
                keep = (vals != 0) & (vals > -np.inf)
                if filter_interacted:
                    keep &= ~np.isin(cols, own)
                cols, vals = cols[keep], vals[keep]
                order = np.argsort(-vals, kind="stable")[:top_k]
                sel, val = cols[order], vals[order]
            n = len(sel)
            with np.errstate(over="ignore"):
                o_ids[r, :n], o_sc[r, :n], o_cnt[r] = sel, val.astype(np.float32), n
        return o_ids, o_sc, o_cnt

    def score_rows(self, n_rows, row_ids, xb, n_items, col_lo, lay, acc_f64, out):
        Wr = self._shard_w(n_items, col_lo, lay)
        ptr, col, val = (t.numpy() for t in xb)
        Xall = sp.csr_matrix((val, col, ptr), shape=(len(ptr) - 1, n_items))
        dt = np.float64 if acc_f64 else np.float32
        S = (Xall.astype(dt) @ Wr.astype(dt)).toarray()[:, col_lo:col_lo + lay["n_cols"]]
        out[:, :lay["n_cols"]] = torch.from_numpy(np.ascontiguousarray(S))

    def merge_topk(self, n_rows, n_lists, top_k, g_ids, g_sc, g_sc64, g_aux, g_cnt, o_ids, o_sc, o_cnt):
        gi, gs, ga, gc = g_ids.numpy(), g_sc.numpy(), g_aux.numpy().view(np.uint32), g_cnt.numpy()
        if g_sc64 is not None:      # include/rtrec_amd.h: the doubles are compared, the returned score is their float32 rounding
            gs = g_sc64.numpy()
        for r in range(n_rows):
            cand = [(gs[l, r, k], ga[l, r, k], gi[l, r, k]) for l in range(n_lists) for k in range(gc[l, r])]
            cand.sort(key=lambda c: (-c[0], -int(c[1]), -int(c[2])))
            cand = cand[:top_k]
            o_cnt[r] = len(cand)
            pad = top_k - len(cand)
            o_ids[r] = torch.tensor([int(c[2]) for c in cand] + [-1] * pad, dtype=torch.int32)
            o_sc[r] = torch.tensor([float(c[0]) for c in cand] + [float("-inf")] * pad, dtype=torch.float64).to(torch.float32)

    def similar_topk(self, queries, W, top_k, ids, sc, cnt):
        n_items = W["cptr"].shape[0] - 1
        Wc = sp.csc_matrix((W["cval"].numpy(), W["crow"].numpy(), W["cptr"].numpy()), shape=(n_items, n_items))
        ids.fill_(-1); sc.fill_(float("-inf"))
        for q, j in enumerate(queries.numpy()):
            oi, ov = so.similar_items(Wc, int(j), top_k=top_k)
            ids[q, :len(oi)] = torch.from_numpy(oi)
            sc[q, :len(oi)] = torch.from_numpy(ov)
            cnt[q] = len(oi)

    def fit_columns_sgd(self, X, n_users, n_items, targets, alpha, l1_ratio, eta0, max_iter, tol, random_state, K):
        """optim="sgd" on the stand-in backend: the oracle's restatement per column, returned in the layout of
        SlimEngine.fit_columns_sgd (items = the K selected features, ascending here: the merge does not care)."""
        Xc = sp.csc_matrix((X["cval"].numpy(), X["crow"].numpy(), X["cptr"].numpy()), shape=(n_users, n_items))
        tg = np.asarray(targets, dtype=np.int64)
        ptr, idx, val, nit = so.fit_columns_sgd(Xc, tg, alpha=alpha, l1_ratio=l1_ratio, eta0=eta0, tol=tol, max_iter=max_iter,
                                                random_state=random_state, nn_feature_selection=K)
        k = min(K, n_items)
        return (torch.from_numpy(tg.astype(np.int32)), torch.from_numpy(idx.reshape(len(tg), k).copy()),
                torch.from_numpy(val.reshape(len(tg), k).copy()), torch.full((len(tg),), k, dtype=torch.int32), nit)
