"""SLIM model: the drop-in for rtrec.models.SLIM (/root/reference/rtrec/models/slim.py:21-149).

Same constructor kwargs (fan out to the interaction store, both Identifiers and SLIMElastic;
unknown keys ignored), same fit / bulk_fit / recommend / recommend_batch / similar_items
behaviour, same pickle payload keys.  The interaction matrix is kept resident in HBM between
calls and scored in place by row id instead of being rebuilt and sliced per request.
"""
from __future__ import annotations

import os
from typing import Any, Dict, Iterable, List, NamedTuple, Optional, Tuple

import numpy as np

from .._native import TOPK_DENSE, TOPK_SPARSE
from ..utils.device_store import DeviceInteractions
from .base import BaseModel
from .internal.slim_elastic import SLIMElastic
from .. import settings


class _UserBatch(NamedTuple):
    """The users of a model-level batch call, split as recommend_batch splits them (SLIM._user_batch)."""
    users: Any              # the int64 array of ids that pass through unmapped, else a list
    B: int
    uid: np.ndarray         # internal user id per user (0 for a cold one)
    cold: np.ndarray        # nobody the model knows: the cold-start list
    regular: np.ndarray     # a row of X: what the device pass serves

    # the two derived views build a new array per access: a caller takes each once, outside its loops
    @property
    def rows(self) -> np.ndarray:
        """The row of X per user as the kernels take it: int32, -1 for a user without one."""
        return np.where(self.regular, self.uid, -1).astype(np.int32)

    @property
    def odd(self) -> np.ndarray:
        """Known, but outside the matrix (a negative id, an id known only through register_user_feature): _recommend_odd_ids."""
        return ~self.cold & ~self.regular


class SLIM(BaseModel):
    def __init__(self, **kwargs: Any):
        super().__init__(**kwargs)
        self.model = SLIMElastic(kwargs)
        self.recorded_item_ids: set = set()
        self._x_on_device: Optional[Tuple[int, float]] = None   # (store version, max_timestamp) of the GPU copy
        self._dev_x: Optional[DeviceInteractions] = None        # X resident in HBM (utils/device_store.py)
        self._factors: Optional[Dict[str, np.ndarray]] = None   # vectors of a factor model the caller attached (attach_factors)
        self._factors_on_device: Any = None                     # (what the engine's resident copy was built for, has-vector mask)
        self._factor_training: Optional[Dict[str, float]] = None   # regularization / alpha (/ solver, cg_steps) of the last fit_factors

    # ------------------------------------------------------------ device-resident X
    def _store_tag(self) -> Any:
        """What a device copy of X must match to be current: the store version, and with time decay also
        max_timestamp (every value is a function of it)."""
        st = self.interactions
        return st.version if st.decay_rate is None else (st.version, st.max_timestamp)

    def _mirror(self, full: bool = False) -> Optional[DeviceInteractions]:
        """The device-resident copy of X, or None where it does not apply (a backend without device arrays).
        Stores with time decay keep their raw values and timestamps resident too and are re-valued on the device
        at every new max_timestamp (utils/device_store.py).  RTREC_AMD_DEVICE_STORE=0 forces the host-export path."""
        if settings.raw("RTREC_AMD_DEVICE_STORE", "1") == "0":
            return None
        be = self.model.engine.be
        if not getattr(be, "supports_device_store", False):
            return None
        if self._dev_x is None:
            self._dev_x = DeviceInteractions(be.torch, be.device)
            self._dev_x.decay_fn = getattr(be, "decay_f32", None)
        return self._dev_x

    def _mirror_synced(self, full: bool = False) -> Optional[DeviceInteractions]:
        """The mirror, brought up to the host store's state (one upload of the store's compacted block -- keys, raw
        values, timestamps -- if it has fallen behind; values are cast / decayed on the device)."""
        mir = self._mirror(full)
        if mir is not None and mir.version != self._store_tag():
            st = self.interactions
            blk = st._compact()
            mir.load_store(blk.key, blk.val, blk.ts if st.decay_rate is not None else None, st.shape[0], st.shape[1],
                           self._store_tag(), rate=st.decay_rate, now=st.max_timestamp)
        return mir

    _MIRROR_APPLY_MAX = 1 << 18     # larger writes (bulk chunks) leave the mirror stale: it is rebuilt on demand

    @property
    def bulk_chunk_rows(self) -> Optional[int]:
        """How many DataFrame rows Recommender hands over per add_interactions_columns call: with the device ingest one
        chunk is one upload + one sort, so the whole frame goes in one piece (64 M rows = 2 GiB of columns)."""
        return (1 << 26) if self._bulk_folder(1 << 26) is not None else None

    def _bulk_folder(self, n: int) -> Any:
        """Bulk batches are sorted, deduplicated and folded on the device (DeviceInteractions.ingest with the backend's
        rtrec_store_fold_device kernel); a batch into an EMPTY store also leaves the mirror in step -- no upload later."""
        from ..utils.interactions import _DEVICE_FOLD_MIN
        st = self.interactions
        if (n < _DEVICE_FOLD_MIN or st.decay_rate is not None or settings.raw("RTREC_AMD_DEVICE_INGEST", "1") == "0"):
            return None
        if self.model._engine is None:
            # ingest alone does not need the GPU (the host store is complete by itself): do not construct the engine --
            # which fails loudly without one -- just to look for a folder
            import torch
            if not torch.cuda.is_available():
                return None
        mir = self._mirror(True)
        fold_fn = None if mir is None else getattr(self.model.engine.be, "fold_pairs", None)
        if fold_fn is None:
            return None
        was_empty = st.is_empty

        def fold(users, items, ts, dl, upsert, lo, hi, lookup):
            res = mir.ingest(users, items, ts, dl, upsert, lo, hi, lookup, fold_fn)
            self._ingested_into_empty = was_empty
            return res
        return fold

    def _ingest(self, interactions: Iterable[Tuple[Any, Any, float, float]], update_interaction: bool
                ) -> Tuple[np.ndarray, np.ndarray]:
        tag0 = self._store_tag()
        uid, iid = super()._ingest(interactions, update_interaction)
        self._stored(tag0, uid, iid)
        return uid, iid

    def _stored(self, tag_before: Any, user_ids: np.ndarray, item_ids: np.ndarray) -> None:
        """A mirror that was in step with the store is advanced by the batch's distinct (user, item)
        pairs -- their new (raw) values and timestamps come from the host store, which owns the semantics."""
        st, mir = self.interactions, self._dev_x
        if mir is not None and mir.ingested is not None:       # the batch was folded on the device
            into_empty, self._ingested_into_empty = getattr(self, "_ingested_into_empty", False), False
            if self._store_tag() != tag_before and (into_empty or mir.version == tag_before):
                mir.adopt_ingested(st.shape[0], st.shape[1], self._store_tag(), merge=not into_empty)
                return
            mir.ingested = None
        if (mir is None or mir.version != tag_before or self._store_tag() == tag_before
                or len(user_ids) > self._MIRROR_APPLY_MAX or settings.raw("RTREC_AMD_DEVICE_STORE", "1") == "0"):
            return
        keys = np.unique(st._keys(user_ids, item_ids))
        _, val, ts = st._lookup(keys)
        if st.decay_rate is None:
            mir.apply(keys >> 32, keys & 0xFFFFFFFF, val.astype(np.float32), st.shape[0], st.shape[1], self._store_tag())
        else:
            mir.apply(keys >> 32, keys & 0xFFFFFFFF, val, st.shape[0], st.shape[1], self._store_tag(), tstamps=ts,
                      now=st.max_timestamp)

    def _device_matrix(self, item_ids: Optional[List[int]]) -> Optional[Dict[str, Any]]:
        """X (or X with only `item_ids`' columns populated) as device arrays, or None -> host export."""
        mir = self._mirror_synced(full=item_ids is None)
        if mir is None:
            return None
        X = dict(mir.full() if item_ids is None else mir.partial(np.asarray(item_ids, dtype=np.int64)))
        X["n_users"], X["n_items"] = mir.n_users, mir.n_items
        return X

    # ------------------------------------------------------------ fit
    def fit(self, interactions: Iterable[Tuple[Any, Any, float, float]], update_interaction: bool = False,
            progress_bar: bool = True) -> "SLIM":
        """Ingest a mini-batch and refit exactly the items it touched (slim.py:29-43): the matrix
        handed to the solver has ONLY those items' columns populated."""
        _, iid = self._ingest(interactions, update_interaction)
        item_ids = np.unique(iid).tolist()
        self._fit_items(item_ids, False, progress_bar)
        return self

    def _fit_items(self, item_ids: List[int], parallel: bool, progress_bar: bool) -> None:
        X = self._device_matrix(item_ids) if item_ids else None
        if X is not None:
            self.model.partial_fit_items_device(X, item_ids)
        else:
            interaction_matrix = self.interactions.to_csc(item_ids)
            self.model.partial_fit_items(interaction_matrix, item_ids, parallel=parallel, progress_bar=progress_bar)
        self._x_on_device = None

    def _record_interactions(self, user_id: int, item_id: int, tstamp: float, rating: float) -> None:
        self.recorded_item_ids.add(item_id)

    def _record_batch(self, user_ids: np.ndarray, item_ids: np.ndarray) -> None:
        self.recorded_item_ids.update(np.unique(item_ids).tolist())

    def _fit_recorded(self, parallel: bool = False, progress_bar: bool = True) -> "SLIM":
        item_ids = sorted(self.recorded_item_ids)
        self._fit_items(item_ids, parallel, progress_bar)
        self.recorded_item_ids.clear()
        return self

    def bulk_fit(self, parallel: bool = False, progress_bar: bool = True) -> "SLIM":
        X = self._device_matrix(None)
        if X is not None:        # resident X: CSR order from the host keys, CSC order by a sort on the device
            self.model.fit_device(X, parallel=parallel)
        else:
            self.model.fit(self.interactions.to_csc(), parallel=parallel, progress_bar=progress_bar)
        self._x_on_device = None
        return self

    # ------------------------------------------------------------ recommend
    def _sync_interactions(self) -> None:
        """Make the GPU copy of X (CSR, decayed to the current max_timestamp) current."""
        stamp = (self.interactions.version, self.interactions.max_timestamp)
        if self._x_on_device != stamp:
            mir = self._mirror(full=True)
            if mir is not None and mir.version == self._store_tag():
                self.model.engine.set_interactions_device(mir.full(), mir.n_users, mir.n_items)
            else:
                self.model.engine.set_interactions(None, self.interactions.to_csr(), need_csc=False)
            self._x_on_device = stamp

    def _recommend(self, user_id: int, candidate_item_ids: Optional[List[int]] = None,
                   user_tags: Optional[List[str]] = None, top_k: int = 10, filter_interacted: bool = True) -> List[int]:
        return self._recommend_hot_batch([user_id], candidate_item_ids=candidate_item_ids, top_k=top_k,
                                         filter_interacted=filter_interacted)[0]

    def _recommend_hot_batch(self, user_ids: List[int], candidate_item_ids: Optional[List[int]] = None,
                             users_tags: Optional[List[List[str]]] = None, top_k: int = 10,
                             filter_interacted: bool = True) -> List[List[int]]:
        if not self.model.is_fitted:
            raise RuntimeError("Model must be fitted before calling batch_recommend.")
        if len(user_ids) == 0:
            return []
        n_users = self.interactions.shape[0]
        ids_arr = np.asarray(user_ids, dtype=np.int64)
        if int(ids_arr.min()) < 0 or int(ids_arr.max()) >= n_users:
            return self._recommend_odd_ids(ids_arr, n_users, candidate_item_ids, top_k, filter_interacted)
        ids, scores, counts = self._hot_topk(ids_arr, candidate_item_ids, top_k, filter_interacted)
        return self.model._format(ids, scores, counts, ret_scores=False)

    def _recommend_hot_arrays(self, user_ids: np.ndarray, candidate_item_ids: Optional[List[int]], top_k: int,
                              filter_interacted: bool) -> Tuple[np.ndarray, np.ndarray]:
        """The kernels' own output -- ids[B, k] and counts[B] as they come off the device in one copy -- with no Python
        object per user or per item (BaseModel.recommend_batch's vectorised route)."""
        if not self.model.is_fitted:
            raise RuntimeError("Model must be fitted before calling batch_recommend.")
        if len(user_ids) == 0:
            return np.empty((0, top_k), np.int32), np.zeros(0, np.int32)
        n_users = self.interactions.shape[0]
        if int(user_ids.min()) < 0 or int(user_ids.max()) >= n_users:
            return super()._recommend_hot_arrays(user_ids, candidate_item_ids, top_k, filter_interacted)
        ids, _, counts = self._hot_topk(user_ids, candidate_item_ids, top_k, filter_interacted)
        return ids, counts

    def _hot_topk(self, ids_arr: np.ndarray, candidate_item_ids: Optional[List[int]], top_k: int, filter_interacted: bool):
        """(ids, scores, counts) arrays for internal user ids inside [0, n_users)."""
        dense_output = not self.item_ids.pass_through
        stamp = (self.interactions.version, self.interactions.max_timestamp)
        n_users = self.interactions.shape[0]
        resident = self._dev_x is not None and self._dev_x.version == self._store_tag()
        if self._x_on_device == stamp or resident or len(ids_arr) * 16 >= n_users:
            # bulk scoring: (re)upload all of X once and score it in place by row id
            self._sync_interactions()
            return self.model._topk(None, candidate_item_ids, top_k, filter_interacted, dense_output, row_ids=ids_arr)
        # online serving after an update: ship only the requested users' rows (like the
        # reference's to_csr(select_users=...), but without the empty rows)
        uniq, inverse = np.unique(ids_arr, return_inverse=True)
        rows, cols, data = self.interactions._triples(select_users=uniq)
        indptr = np.zeros(len(uniq) + 1, dtype=np.int64)
        indptr[1:] = np.bincount(np.searchsorted(uniq, rows), minlength=len(uniq))
        np.cumsum(indptr, out=indptr)
        from scipy.sparse import csr_matrix
        Xb = csr_matrix((data.astype(np.float32), cols.astype(np.int32), indptr.astype(np.int32)),
                        shape=(len(uniq), self.interactions.shape[1]))
        ids, scores, counts = self.model._topk(Xb, candidate_item_ids, top_k, filter_interacted, dense_output)
        return ids[inverse], scores[inverse], counts[inverse]

    def _recommend_odd_ids(self, ids: np.ndarray, n_users: int, candidate_item_ids: Optional[List[int]], top_k: int,
                           filter_interacted: bool) -> List[List[int]]:
        """Internal user ids outside [0, n_users) -- a negative integer user, or a user known only through
        register_user_feature -- never reach the device.  They get what the reference's scipy row indexing
        of to_csr(select_users=...) gives them (slim.py:93, slim_elastic.py:707): IndexError beyond the
        matrix, and for a negative id the row it wraps around to, which is populated only if that user is
        in the same batch."""
        bad = ids[(ids >= n_users) | (ids < -n_users)]
        if len(bad):
            raise IndexError(f"index ({int(bad[0])}) out of range")
        regular = set(ids[ids >= 0].tolist())
        rows = np.where(ids < 0, ids + n_users, ids)
        live = np.array([(i >= 0) or (int(w) in regular) for i, w in zip(ids.tolist(), rows.tolist())], dtype=bool)
        out: List[List[int]] = [[] for _ in ids]
        if live.any():
            got = self._recommend_hot_batch(rows[live].tolist(), candidate_item_ids=candidate_item_ids, top_k=top_k,
                                            filter_interacted=filter_interacted)
            for p, row in zip(np.flatnonzero(live).tolist(), got):
                out[p] = row
        if candidate_item_ids is not None and not live.all():
            # an all-zero row still ranks the candidates (scores 0): argsort(...)[-k:][::-1], slim_elastic.py:730-733
            k = min(top_k, len(candidate_item_ids))
            zero_row = [candidate_item_ids[j] for j in range(len(candidate_item_ids) - 1, len(candidate_item_ids) - 1 - k, -1)]
            for p in np.flatnonzero(~live).tolist():
                out[p] = list(zero_row)
        elif not self.item_ids.pass_through and not live.all():
            # dense mode ranks every item of an all-zero row too: highest ids first (stable-argsort rule, D1)
            n_items = self.model.n_items_fitted
            k = min(top_k, n_items)
            for p in np.flatnonzero(~live).tolist():
                out[p] = list(range(n_items - 1, n_items - 1 - k, -1))
        return out

    # ------------------------------------------------------------ evaluate on the device
    @staticmethod
    def _internal_ids(ident, values: np.ndarray, what: str) -> np.ndarray:
        """Identifier.get_id over the distinct raw ids of an evaluation frame's column: int64 internal ids, -1 for a value
        the identifier has never seen.  Integer pass-through ids are returned as they are (one vectorised step)."""
        if ident.pass_through and not ident.force_identify:
            if values.dtype.kind not in "iu":
                raw = values.tolist()
                if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in raw):
                    raise ValueError(f"on_device evaluation: the {what} column mixes integer ids with other values")
                values = np.fromiter((int(v) for v in raw), dtype=np.int64, count=len(raw))
            return values.astype(np.int64)
        # items are only tested for membership (an id of another kind is in no recommendation); users go through get_id
        # like recommend_batch's own loop, with its "mixed types" error
        get = ident.obj_to_id.get if what == "item" else ident.get_id
        return np.fromiter((-1 if (i := get(v)) is None else i for v in values.tolist()), dtype=np.int64, count=len(values))

    def _evaluate_device(self, users: np.ndarray, items: np.ndarray, size: int, filter_interacted: bool,
                         want_rel: bool = False, diversity: float = 0.0, pool: int = 50, list_quality: bool = False):
        """Recommender.evaluate without leaving the device: every user of the frame scored in ONE pass whose lists stay in
        HBM, rank_metrics_kernel (csrc/rank_metrics.hip) on (lists, ground truth), and only the per-user figures come back.
        Returns (users in evaluation order, metrics[n, 8] float64 in utils.metrics.METRIC_COLUMNS order, tp[n] int32,
        rel[n] uint64 or None).  Known users get recommend_batch's hot lists, unknown ones its cold-start list.  What this
        path does not serve is refused with ValueError -- the caller evaluates on the host instead.  With several ranks the
        scoring pass is the usual collective and every rank computes the same figures.
        `diversity > 0`: known users are judged on recommend_diverse_batch(top_k=size, pool, diversity)'s lists instead, with
        its refusals.  `list_quality=True`: the same lists also go through list_quality_kernel (csrc/list_quality.hip) in the
        same pass, and a fifth element is returned: numpy (n, sim_sum, linked, weight_sum, exposure[W's n_items])."""
        from ..backend import HipBackend
        from ..utils.metrics import discount_tables, ground_truth_csr
        eng = self.model.engine
        be = eng.be
        if not isinstance(be, HipBackend):
            raise ValueError("on_device evaluation needs the HIP backend; this model scores through another one")
        if not 1 <= size <= 64:
            raise ValueError(f"on_device evaluation serves recommend_size 1..64, got {size}")
        if (type(self).handle_unknown_user is not BaseModel.handle_unknown_user
                or type(self)._recommend_cold_batch is not BaseModel._recommend_cold_batch):
            raise ValueError("on_device evaluation: this model serves unknown users through hooks of its own")
        for name, col in (("user", users), ("item", items)):
            if col.dtype.kind not in "iuO":
                raise ValueError(f"on_device evaluation takes integer or object id columns; the {name} column is {col.dtype}")
        lam = None
        if float(diversity) != 0.0:                                         # (a NaN is not 0: _mmr_lambda refuses it)
            _, pool, lam = self._diverse_args("on_device evaluation with diversity", size, pool, diversity)
        if not self.model.is_fitted:
            raise RuntimeError("Model must be fitted before calling batch_recommend.")
        n_users, n_items = self.interactions.shape[0], self.model.n_items_fitted

        def user_index(values: np.ndarray) -> np.ndarray:
            ids = self._internal_ids(self.user_ids, values, "user")
            if self.user_ids.pass_through:
                if (ids < 0).any():
                    raise ValueError("on_device evaluation: negative integer user ids are served by the host path only")
                ids = np.where(ids > self.interactions.max_user_id, -1, ids)     # BaseModel._known_user_id: a cold-start user
            return ids

        def item_index(values: np.ndarray) -> np.ndarray:
            ids = self._internal_ids(self.item_ids, values, "item")
            return np.where((ids >= 0) & (ids < 2 ** 31), ids, -1)          # (beyond int32: no list can hold it)

        eval_users, rows, truth_ptr, truth_items, truth_len = ground_truth_csr(users, items, user_index, item_index)
        n = len(eval_users)
        if n == 0:
            none = (eval_users, np.empty((0, 8), np.float64), np.empty(0, np.int32), (np.empty(0, np.uint64) if want_rel else None))
            return none if not list_quality else none + ((np.empty(0, np.int32), np.empty(0, np.float32), np.empty(0, np.int32),
                                                          np.empty(0, np.float32), np.zeros(n_items, np.int32)),)
        hot = rows >= 0
        hot_rows = rows[hot]
        if len(hot_rows) and int(hot_rows.max()) >= n_users:
            raise ValueError("on_device evaluation: a user known only through register_user_feature is served by the host path only")
        mode = self._topk_mode()
        top_k = min(size, n_items)
        self.model._sync_weights()
        if top_k < 1 or not eng.topk_supported(top_k, mode):
            raise ValueError(f"on_device evaluation: the fused top-k kernels do not serve recommend_size {size} for this model")
        k_pool = 0
        if lam is not None:
            eng._whole_w("diversify")
            k_pool = self._pool_width("on_device evaluation with diversity", pool, mode)
        if list_quality:
            eng._whole_w("list_quality")
        torch = be.torch
        ids = cnt = None
        if len(hot_rows):
            self._sync_interactions()
            ids, cnt = self._hot_lists_device(hot_rows, top_k, lam, k_pool, filter_interacted, mode)
        if len(hot_rows) < n or top_k < size or not ids.is_contiguous():
            # the rows of unknown users (recommend_batch gives them all the hot-items list) and lists narrower than `size`
            # are placed on the device
            all_ids = torch.full((n, size), -1, dtype=torch.int32, device=be.device)
            all_cnt = be.zeros((n,), torch.int32)
            if ids is not None:
                pos = be.to_dev(np.flatnonzero(hot))
                all_ids[pos, :top_k] = ids
                all_cnt[pos] = cnt
            # (every user here is hot or cold: negative ids and ids beyond the matrix were refused above)
            self._fill_unserved_device(_UserBatch(eval_users, n, np.maximum(rows, 0), ~hot, hot), size, filter_interacted, all_ids, all_cnt)
            ids, cnt = all_ids, all_cnt
        discount, ideal = discount_tables(size)
        d_metrics = be.empty((n, 8), torch.float64)
        d_tp = be.empty((n,), torch.int32)
        d_rel = be.empty((n,), torch.int64)
        be.ops.rank_metrics(ids, cnt.contiguous(), be.to_dev(truth_ptr), be.to_dev(truth_items), be.to_dev(truth_len),
                            be.to_dev(discount), be.to_dev(ideal), size, d_metrics, d_tp, d_rel)
        rel = d_rel.cpu().numpy().view(np.uint64) if want_rel else None
        if not list_quality:
            return eval_users, d_metrics.cpu().numpy(), d_tp.cpu().numpy(), rel
        self._sync_interactions()                                           # (the novelty table is X's, whoever is in the frame)
        exposure = be.zeros((eng._whole_w("list_quality").n_items,), torch.int32)
        quality = eng.list_quality_device(ids, cnt.contiguous(), eng.item_novelty_device(), exposure)
        return (eval_users, d_metrics.cpu().numpy(), d_tp.cpu().numpy(), rel,
                tuple(t.cpu().numpy() for t in quality) + (exposure.cpu().numpy(),))

    # ------------------------------------------------------------ explanations (an extension: the reference has none)
    def explain_batch(self, users: List[Any], items: Optional[List[List[Any]]] = None, top_k: int = 10, top_m: int = 3,
                      filter_interacted: bool = True, as_arrays: bool = False) -> Any:
        """Why each item is recommended: in SLIM score(u, i) = sum_j X[u, j] * W[j, i] over the items j the user interacted
        with, and the largest terms are the "because you interacted with ..." of a recommendation (csrc/explain.hip).

        `items=None`: recommend `top_k` items per user and explain them in one device pass over the resident X -- the lists
        go from the scoring kernels to the explanation kernel without visiting the host.  `items` = one list of raw item ids
        per user (at most 64 each): explain those instead, e.g. a list that was served earlier; an item the model does not
        know gets an empty explanation.

        Per (user, item) the contributing items are the j stored in both the user's row of X and column i of W, the
        contribution of j is the float32 product x_uj * w_ji (one rounding), and the reasons are the `top_m` (1..32)
        contributing items by contribution descending, the lower item id first among equal ones; negative contributions take
        part (filter by sign if only positive reasons are wanted).  A contribution that is NaN (an infinite rating next to a
        zero weight) counts in the support and is never a reason; +-inf are numbers.  For a float32 W, adding ALL contributions of a pair in
        ascending item order in float32 gives exactly the score `recommend` ranks it by.  Unknown users get their cold-start
        list with empty reasons; users outside the matrix follow `recommend_batch`'s rules for the list and get empty reasons.

        Returns, per user, [(item, [(reason_item, contribution), ...]), ...] with raw ids and float contributions -- or with
        `as_arrays=True` (ids[B, k], counts[B], reason_ids[B, k, top_m], contributions[B, k, top_m], support[B, k]): row b is
        valid up to counts[b], support = the number of contributing items of the pair (it may exceed top_m), unused slots
        hold -1 / -inf.  The id arrays hold INTERNAL item ids: for integer ids those are the raw ids, for a model with string
        ids map them with `model.item_ids.get`."""
        self._require_fitted("explain_batch")
        users = self._user_list(users)
        B, m = len(users), int(top_m)
        if items is not None:
            items = [list(row) for row in items]
            if len(items) != B:
                raise ValueError(f"items must hold one list per user: {len(items)} lists for {B} users")
            K = max([len(row) for row in items] + [1])
        else:
            K = int(top_k)
        if not 1 <= K <= 64 or not 1 <= m <= 32:
            raise ValueError(f"explain_batch serves lists of 1..64 items and top_m in 1..32, got {K} and {m}")
        ids = np.full((B, K), -1, dtype=np.int64)
        counts = np.zeros(B, dtype=np.int32)
        r_ids = np.full((B, K, m), -1, dtype=np.int64)
        contrib = np.full((B, K, m), -np.inf, dtype=np.float32)
        support = np.zeros((B, K), dtype=np.int32)
        eng = self.model.engine
        n_items = self.model.n_items_fitted
        batch = self._user_batch(users)
        regular = batch.regular
        if B:
            self.model._sync_weights()
            eng._whole_w("explain")                # a W that cannot be explained is refused whatever the batch holds
        if items is not None:                      # brought lists: nothing is filled in, a user without a row has no reasons
            for b, row in enumerate(items):
                counts[b] = len(row)
                ids[b, :len(row)] = self._ids_or_minus_one(row, self.item_ids.get_id, n_items)
            if regular.any():
                self._sync_interactions()
                r_ids[:], contrib[:], support[:] = eng.explain_rows(batch.rows, ids, counts, m)
        elif B:
            self._fill_unserved(batch, K, filter_interacted, ids, counts)      # (no scores: the reasons stay empty)
            k = min(K, n_items)
            if regular.any() and k >= 1:
                self._sync_interactions()
                rows = batch.uid[regular].astype(np.int32)
                mode = self._topk_mode()
                if eng.topk_supported(k, mode):
                    d_rows = eng._up(rows)
                    d_ids, _, d_cnt = eng.score_topk_device(None, len(rows), k, filter_interacted, mode, d_rows=d_rows)
                    out = eng.explain_device(d_rows, len(rows), None, d_ids, d_cnt, m)
                    h_ids, h_cnt = d_ids.cpu().numpy(), d_cnt.cpu().numpy()
                    h_r, h_c, h_s = (t.cpu().numpy() for t in out)
                else:                            # a catalogue the fused top-k does not serve: lists selected on the host
                    h_ids, _, h_cnt = self.model._topk(None, None, k, filter_interacted, not self.item_ids.pass_through, row_ids=rows)
                    h_r, h_c, h_s = eng.explain_rows(rows, h_ids, h_cnt, m)
                pos = np.flatnonzero(regular)
                ids[pos, :k], counts[pos] = h_ids, h_cnt
                r_ids[pos, :k], contrib[pos, :k], support[pos, :k] = h_r, h_c, h_s
        if as_arrays:
            return ids, counts, r_ids, contrib, support
        raw_of = self._raw_of(self.item_ids)
        id_rows, cnts, reason_rows, contrib_rows = ids.tolist(), counts.tolist(), r_ids.tolist(), contrib.tolist()
        n_reasons = (r_ids >= 0).sum(axis=2).tolist()      # the reasons present: a NaN contribution counts in support, not here
        out_rows: List[List[Tuple[Any, List[Tuple[Any, float]]]]] = []
        for b in range(B):
            row = []
            for p_ in range(cnts[b]):
                item = items[b][p_] if items is not None else raw_of(id_rows[b][p_])
                row.append((item, [(raw_of(reason_rows[b][p_][q]), contrib_rows[b][p_][q]) for q in range(n_reasons[b][p_])]))
            out_rows.append(row)
        return out_rows

    def explain(self, user: Any, items: Optional[List[Any]] = None, top_k: int = 10, top_m: int = 3,
                filter_interacted: bool = True) -> List[Tuple[Any, List[Tuple[Any, float]]]]:
        """explain_batch for one user: [(item, [(reason_item, contribution), ...]), ...]."""
        return self.explain_batch([user], None if items is None else [list(items)], top_k=top_k, top_m=top_m,
                                  filter_interacted=filter_interacted)[0]

    # ------------------------------------------------------------ rerank per-user candidate lists (an extension)
    RERANK_MAX_LIST = 1024      # list length rtrec_slim_score_pairs ranks

    @staticmethod
    def _ids_or_minus_one(values: Any, known, bound: Optional[int] = None) -> np.ndarray:
        """Raw ids to an int64 array of internal ids through `known` (item_ids.get_id, _known_user_id): -1 for an id the model
        does not know, an id of the other kind, and an internal id outside [0, bound)."""
        values = values.tolist() if isinstance(values, np.ndarray) else list(values)
        out = np.full(len(values), -1, dtype=np.int64)
        for p_, raw in enumerate(values):
            try:
                i = known(raw)
            except (ValueError, TypeError):       # an id of the other kind: nobody / nothing the model knows
                i = None
            if i is not None and 0 <= i and (bound is None or i < bound):
                out[p_] = i
        return out

    @staticmethod
    def _raw_of(id_map: Any):
        """Internal id -> raw id: the identity for ids that pass through unmapped."""
        return (lambda i: i) if id_map.pass_through else id_map.get

    # ------------------------------------------------------------ what the model-level batch calls share
    def _require_fitted(self, what: str) -> None:
        if not self.model.is_fitted:
            raise RuntimeError(f"Model must be fitted before calling {what}.")

    def _topk_mode(self) -> int:
        """The mode `recommend` ranks this model by: stored non-zero products for integer item ids, every item otherwise."""
        return TOPK_SPARSE if self.item_ids.pass_through else TOPK_DENSE

    def _user_list(self, users: Any) -> Any:
        """`users` as the int64 array of ids that pass through unmapped, else as a list: what len() and a second pass need."""
        arr = self._int_user_array(users)
        return arr if arr is not None else list(users)

    def _user_batch(self, users: Any) -> _UserBatch:
        """The hot / cold split of recommend_batch -- one compare for integer pass-through ids, `_known_user_id` per user
        otherwise (with its "mixed types" error) -- and who of the hot users has a row of X."""
        users = self._user_list(users)
        if isinstance(users, np.ndarray):
            uid, cold = users, users > self.interactions.max_user_id
        else:
            known = [self._known_user_id(u) for u in users]
            cold = np.fromiter((u is None for u in known), dtype=bool, count=len(known))
            uid = np.fromiter((0 if u is None else u for u in known), dtype=np.int64, count=len(known))
        regular = ~cold & (uid >= 0) & (uid < self.interactions.shape[0])
        return _UserBatch(users, len(users), uid, cold, regular)

    def _unserved_lists(self, batch: _UserBatch, top_k: int, filter_interacted: bool,
                        cold_candidates: Optional[List[int]] = None, unserved: Optional[np.ndarray] = None):
        """(positions in the batch, internal item ids) of the lists a device pass over the regular users leaves open: the
        cold-start list once for all cold users (positions: an index array), then `_recommend_odd_ids`' list per user
        outside the matrix (position: an int) -- asked for ALL known users, so that a negative id still wraps to a row of
        the same batch, and raising its IndexError for an id beyond the matrix.  `unserved` (a mask) gets the cold-start
        list instead of `cold`, among `cold_candidates`, and nobody is asked about then."""
        cold = batch.cold if unserved is None else unserved
        if cold.any():
            yield np.flatnonzero(cold), self._recommend_cold_batch([None], candidate_item_ids=cold_candidates, top_k=top_k)[0][:top_k]
        odd = batch.odd
        if unserved is None and odd.any():
            lists = self._recommend_odd_ids(batch.uid[~batch.cold], self.interactions.shape[0], None, top_k, filter_interacted)
            for b, row in zip(np.flatnonzero(~batch.cold).tolist(), lists):
                if odd[b]:
                    yield b, row

    def _fill_unserved(self, batch: _UserBatch, top_k: int, filter_interacted: bool, ids: np.ndarray, counts: np.ndarray,
                       scores: Optional[np.ndarray] = None, cold_candidates: Optional[List[int]] = None,
                       unserved: Optional[np.ndarray] = None) -> None:
        """_unserved_lists into the padded host outputs `ids` [B, K] / `counts` [B]; the listed entries of `scores` get 0.0."""
        for pos, row in self._unserved_lists(batch, top_k, filter_interacted, cold_candidates, unserved):
            ids[pos, :len(row)] = np.asarray(row, dtype=np.int64)
            counts[pos] = len(row)
            if scores is not None:
                scores[pos, :len(row)] = 0.0

    def _fill_unserved_device(self, batch: _UserBatch, top_k: int, filter_interacted: bool, d_ids: Any, d_cnt: Any) -> None:
        """_unserved_lists into the int32 device tensors `d_ids` [B, K] / `d_cnt` [B]: one upload per list (the cold-start
        list is broadcast on the device) and none for an empty one."""
        be = self.model.engine.be
        for pos, row in self._unserved_lists(batch, top_k, filter_interacted):
            if row:
                at = pos if isinstance(pos, int) else be.to_dev(pos)
                d_ids[at, :len(row)] = be.to_dev(np.asarray(row, dtype=np.int32))
                d_cnt[at] = len(row)

    @staticmethod
    def _padded(B: int, K: int, *dtypes: Any) -> Tuple[np.ndarray, ...]:
        """The [B, K] outputs of a batch call before anything is listed -- -1 for int64 ids, -inf for float values, 0 for an
        int32 source -- and counts[B] = 0 behind them."""
        empty = {np.int64: -1, np.float32: -np.inf, np.float64: -np.inf, np.int32: 0}
        return tuple(np.full((B, K), empty[dt], dtype=dt) for dt in dtypes) + (np.zeros(B, dtype=np.int32),)

    def _lists_tail(self, ids: np.ndarray, counts: np.ndarray, scores: Optional[np.ndarray] = None, id_map: Any = None,
                    keep_raw: Optional[np.ndarray] = None) -> List[List[Any]]:
        """The list form of padded outputs: per row the first counts[b] ids mapped to raw ids through `id_map` (default: the
        item ids; the rows of the mask `keep_raw` stay as they are), as (id, score) tuples where `scores` is given.  One
        tolist() per array, so the elements are Python ints and floats."""
        id_map = self.item_ids if id_map is None else id_map
        get = None if id_map.pass_through else id_map.get             # (ids that pass through unmapped are their own raw ids)
        id_rows, cnts = ids.tolist(), counts.tolist()
        sc_rows = None if scores is None else scores.tolist()
        as_is = None if keep_raw is None or get is None else keep_raw.tolist()
        out: List[List[Any]] = []
        for b, n in enumerate(cnts):
            row = id_rows[b][:n]
            if get is not None and not (as_is and as_is[b]):
                row = [get(i) for i in row]
            out.append(row if sc_rows is None else list(zip(row, sc_rows[b])))
        return out

    def rerank_batch(self, users: List[Any], candidates: List[List[Any]], top_k: Optional[int] = None,
                     filter_interacted: bool = False, ret_scores: bool = False, as_arrays: bool = False) -> Any:
        """The second stage of a two-stage recommender: `candidates` holds one list of raw item ids PER USER (from a retrieval
        stage, a rule, what was shown, 1 positive + 99 sampled negatives), and every list is scored and ordered by
        score(u, i) = sum_j X[u, j] * W[j, i] in one device pass over the resident X (csrc/score_pairs.hip) -- where
        `recommend_batch(candidate_items=...)` takes one list shared by all users.

        For a float32 W, `rerank_batch(users, candidates, top_k)[b] == recommend(users[b], candidate_items=candidates[b],
        top_k=top_k)` for every user: raw candidates the model does not know are dropped from that user's list (unmapped ids,
        integer ids above `max_item_id`), duplicated candidates are separate entries, the later entry comes first among equal
        scores, NaN scores are never listed, and a cold-start user gets what `recommend` gives them -- the hot items that are
        in their list, as `recommend` returns them.  The one exception: a list that is empty after mapping yields [] (the
        reference turns it into "no candidates" and `recommend` then ranks the whole catalogue, which is not what a rerank
        call wants).  With a float64 W (serial fit) `recommend` accumulates in double while this call adds the float32
        products in float32, so last bits and the order of near-ties may differ.  Candidates beyond the fitted W (ingested,
        never fitted) and users without a row in X (negative ids, ids known only through register_user_feature) are served
        as an item without a column / a user without interactions instead of `recommend`'s wrap-around and IndexError.

        `top_k=None` ranks the whole list; `filter_interacted` (default off, as `recommend` ignores it for candidate lists)
        leaves out the candidates stored in the user's row of X.  A list longer than 1024 raises ValueError.  With integer
        item ids `candidates` may be one [B, k] integer array instead of B lists: it is mapped without a Python loop.

        Returns one list of raw item ids per user in rank order -- of (item, score) tuples with `ret_scores` -- or with
        `as_arrays=True` (ids[B, top_k], scores[B, top_k], counts[B]): row b is valid up to counts[b], unused slots hold
        -1 / -inf, and the ids are INTERNAL item ids (for integer ids the raw ids; map string ids with `model.item_ids.get`)."""
        self._require_fitted("rerank_batch")
        users = self._user_list(users)
        B = len(users)
        lim = 2 ** 31 - 1
        if (isinstance(candidates, np.ndarray) and candidates.ndim == 2 and candidates.dtype.kind in "iu"
                and self.item_ids.pass_through is True and not self.item_ids.force_identify):
            # integer ids that pass through unmapped, as one [B, k] array: `_candidate_ids` for all lists at once -- an id above
            # max_item_id is dropped and the rest of its list moves up
            if candidates.shape[0] != B:
                raise ValueError(f"candidates must hold one list per user: {candidates.shape[0]} lists for {B} users")
            known = candidates <= self.interactions.max_item_id
            ids = np.take_along_axis(candidates, np.argsort(~known, axis=1, kind="stable"), axis=1)
            counts = known.sum(axis=1).astype(np.int32)
            ids = np.where((np.arange(ids.shape[1])[None, :] < counts[:, None]) & (ids >= 0) & (ids < lim), ids, -1).astype(np.int32)
        else:
            lists = [self._candidate_ids(list(c)) or [] for c in candidates]
            if len(lists) != B:
                raise ValueError(f"candidates must hold one list per user: {len(lists)} lists for {B} users")
            counts = np.fromiter((len(c) for c in lists), dtype=np.int32, count=B)
            ids = np.full((B, int(counts.max()) if B else 0), -1, dtype=np.int32)
            for b, row in enumerate(lists):
                ids[b, :len(row)] = [i if 0 <= i < lim else -1 for i in row]
        K = int(counts.max()) if B else 0
        ids = ids[:, :K]
        if K > self.RERANK_MAX_LIST:
            raise ValueError(f"rerank_batch ranks lists of up to {self.RERANK_MAX_LIST} candidates, got one of {K}: split it, or "
                             "score it with score_pairs and sort on the host")
        k = K if top_k is None else max(0, min(int(top_k), K))
        out_ids, out_sc, out_cnt = self._padded(B, k, np.int64, np.float32)
        batch = self._user_batch(users)
        cold = batch.cold
        if B:
            self.model._sync_weights()
            self.model.engine._whole_w("score_pairs")    # a W that cannot be served is refused whatever the batch holds
        hot = np.flatnonzero(~cold)
        if len(hot) and k > 0:                        # (a known user outside the matrix is scored as one without interactions)
            all_hot = len(hot) == B
            h_ids, rows = (ids, batch.rows) if all_hot else (np.ascontiguousarray(ids[hot]), batch.rows[hot])
            self._sync_interactions()
            scores, _, order, cnt = self.model.engine.score_pairs_rows(rows, h_ids, counts if all_hot else counts[hot], k,
                                                                       filter_interacted)
            live = order >= 0
            pos = np.where(live, order, 0)
            out_ids[hot] = np.where(live, np.take_along_axis(h_ids, pos, axis=1), -1)
            out_sc[hot] = np.where(live, np.take_along_axis(scores, pos, axis=1), -np.inf)
            out_cnt[hot] = cnt
        for b in np.flatnonzero(cold).tolist():       # BaseModel.recommend's cold-start branch, on this user's own list
            mine = ids[b, :counts[b]].tolist()
            if not mine or k == 0:
                continue
            hot_items = self.interactions.get_hot_items(None if top_k is None else int(top_k), filter_interacted=False)
            row = [i for i in hot_items if i in mine][:k]
            out_ids[b, :len(row)], out_sc[b, :len(row)], out_cnt[b] = row, 0.0, len(row)
        if as_arrays:
            return out_ids, out_sc, out_cnt
        # a cold user's ids stay unmapped, as the reference's `recommend` returns its hot items (base.py:207-210)
        return self._lists_tail(out_ids, out_cnt, out_sc if ret_scores else None, keep_raw=cold)

    def rerank(self, user: Any, candidates: List[Any], top_k: Optional[int] = None, filter_interacted: bool = False,
               ret_scores: bool = False) -> List[Any]:
        """rerank_batch for one user: the user's candidates in rank order, or (item, score) tuples."""
        return self.rerank_batch([user], [list(candidates)], top_k=top_k, filter_interacted=filter_interacted,
                                 ret_scores=ret_scores)[0]

    def score_pairs(self, users: Any, items: Any, as_arrays: bool = False) -> Any:
        """score(u, i) = sum_j X[u, j] * W[j, i] for the pairs (users[p], items[p]) of two equal-length sequences of raw ids:
        the score `recommend` ranks the pair by (for a float32 W, bit for bit), as a feature for a learned ranker or for
        logging what was shown.  Returns `scores` (float32, one per pair), or `(scores, support)` with `as_arrays=True`:
        support = the number of items j the sum runs over.  A pair with an unknown user or an unknown item has score 0.0 and
        support -1; a known pair without common evidence has score 0.0 and support 0.  The pairs are grouped by user on the
        host (one stable argsort), go through the kernel as per-user lists of at most 1024 (csrc/score_pairs.hip, no ranking)
        over the resident X, and come back in the caller's order."""
        if not self.model.is_fitted:
            raise RuntimeError("Model must be fitted before calling score_pairs.")
        users = users if isinstance(users, np.ndarray) else list(users)
        items = items if isinstance(items, np.ndarray) else list(items)
        n = len(users)
        if len(items) != n:
            raise ValueError(f"users and items must have one length: {n} users and {len(items)} items")
        scores = np.zeros(n, dtype=np.float32)
        support = np.full(n, -1, dtype=np.int32)
        n_users, n_items = self.interactions.shape[0], self.model.n_items_fitted
        uid = self._ids_or_minus_one(users, self._known_user_id, n_users)
        iid = self._ids_or_minus_one(items, self.item_ids.get_id, n_items)
        if n:
            self.model._sync_weights()
            self.model.engine._whole_w("score_pairs")
        valid = np.flatnonzero((uid >= 0) & (iid >= 0))
        if len(valid):
            L = self.RERANK_MAX_LIST
            by_user = valid[np.argsort(uid[valid], kind="stable")]
            u_sorted = uid[by_user]
            first = np.flatnonzero(np.r_[True, u_sorted[1:] != u_sorted[:-1]])       # where each user's run starts
            run = np.diff(np.r_[first, len(by_user)])
            in_run = np.arange(len(by_user)) - np.repeat(first, run)
            row_base = np.r_[0, np.cumsum((run + L - 1) // L)]                       # a user with more than L pairs takes several rows
            row = np.repeat(row_base[:-1], run) + in_run // L
            col = in_run % L
            n_rows, width = int(row_base[-1]), int(min(L, run.max()))
            ids = np.full((n_rows, width), -1, dtype=np.int32)
            ids[row, col] = iid[by_user]
            counts = np.bincount(row, minlength=n_rows).astype(np.int32)
            rows = np.zeros(n_rows, dtype=np.int64)
            rows[row] = u_sorted
            self._sync_interactions()
            sc, su, _, _ = self.model.engine.score_pairs_rows(rows, ids, counts, 0, False)
            scores[by_user], support[by_user] = sc[row, col], su[row, col]
        return (scores, support) if as_arrays else scores

    # ------------------------------------------------------------ catalogue ranks (an extension: the reference has none)
    def _catalogue_ranks(self, uid: np.ndarray, tg_ptr: np.ndarray, iid: np.ndarray, filter_interacted: bool):
        """(above, tied, score, competing) of SlimEngine.catalogue_ranks_rows for the internal user ids `uid` (a user without a
        row in X scores 0 everywhere) and internal item ids `iid` (-1: no column), in the mode `recommend` ranks this model by."""
        self.model._sync_weights()
        self.model.engine._whole_w("catalogue_ranks")     # a W that cannot be served is refused whatever the batch holds
        if len(uid) == 0:
            return np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, np.float64), np.empty(0, np.int32)
        self._sync_interactions()
        n_users = self.interactions.shape[0]
        rows = np.where((uid >= 0) & (uid < n_users), uid, -1)
        return self.model.engine.catalogue_ranks_rows(rows, tg_ptr, iid, filter_interacted, self._topk_mode())

    def rank_items_batch(self, users: List[Any], items: List[List[Any]], filter_interacted: bool = True,
                         as_arrays: bool = False) -> Any:
        """At which position of the WHOLE catalogue does each of `items[b]` (raw ids) stand for `users[b]`: the exact rank a
        held-out item has, without a sort and without the score matrix leaving the device.  The user's score row is the one
        `recommend` ranks by (float64 for a float64 W); csrc/catalogue_ranks.hip counts, per item, the competing items that
        score higher (`above`) and the same (`tied`), and per user the competing items (`competing`).  An item competes as in
        `recommend(filter_interacted=...)`: its score is not NaN, the user has not interacted with it (when filtering), and
        -- for integer item ids, where `recommend` lists stored non-zero products only -- its score is not 0.  With no tie,
        `recommend(user, top_k=K)` holds the item at position `above` whenever above < K; with ties it stands somewhere in
        above .. above + tied.  An item that does not compete has above = -1, tied = 0 and can never be listed; its score is
        still returned.  An item the model does not know (no column in W) has -1 / 0 / -inf; a cold-start user (nothing
        `recommend` could rank) has -1 / 0 / -inf for every item and competing = 0.  The other items of the same list
        compete like any item.

        Returns one dict per user: {"items": the raw ids as given, "above": [...], "tied": [...], "score": [...],
        "competing": n} -- or with `as_arrays=True` (ptr[B + 1] int64, above int32, tied int32, score float64, competing[B]
        int32): user b's items are the slots ptr[b] .. ptr[b + 1], in the order given."""
        self._require_fitted("rank_items_batch")
        users = self._user_list(users)
        lists = [c.tolist() if isinstance(c, np.ndarray) else list(c) for c in items]
        B = len(users)
        if len(lists) != B:
            raise ValueError(f"items must hold one list per user: {len(lists)} lists for {B} users")
        ptr = np.zeros(B + 1, dtype=np.int64)
        np.cumsum([len(c) for c in lists], out=ptr[1:])
        flat = [x for c in lists for x in c]
        iid = self._ids_or_minus_one(flat, self.item_ids.get_id, self.model.n_items_fitted)
        _, _, uid, cold, _ = self._user_batch(users)
        iid = np.where(np.repeat(cold, np.diff(ptr)), -1, iid)             # a cold user's items are nobody's
        above, tied, score, competing = self._catalogue_ranks(np.where(cold, -1, uid), ptr, iid, filter_interacted)
        competing = np.where(cold, 0, competing).astype(np.int32)
        if as_arrays:
            return ptr, above, tied, score, competing
        a, t, s, c = above.tolist(), tied.tolist(), score.tolist(), competing.tolist()
        return [{"items": lists[b], "above": a[ptr[b]:ptr[b + 1]], "tied": t[ptr[b]:ptr[b + 1]], "score": s[ptr[b]:ptr[b + 1]],
                 "competing": c[b]} for b in range(B)]

    def rank_items(self, user: Any, items: List[Any], filter_interacted: bool = True) -> Dict[str, Any]:
        """rank_items_batch for one user: {"items", "above", "tied", "score", "competing"}."""
        return self.rank_items_batch([user], [list(items)], filter_interacted=filter_interacted)[0]

    def _evaluate_catalogue(self, users: np.ndarray, items: np.ndarray, filter_interacted: bool):
        """The device side of Recommender.evaluate_catalogue: (users evaluated, tg_ptr, above, tied, score, competing,
        unknown_items, skipped_users).  Per user of the frame (sorted, missing keys dropped, as evaluate orders them) the
        targets are the distinct held-out items with a column in W; frame rows whose item has none are counted in
        unknown_items; users without a row in X or without a target left are counted in skipped_users and left out."""
        from ..utils.metrics import _distinct, _missing, ground_truth_csr
        if not self.model.is_fitted:
            raise RuntimeError("Model must be fitted before calling evaluate_catalogue.")
        n_users, n_items = self.interactions.shape[0], self.model.n_items_fitted

        def user_index(values: np.ndarray) -> np.ndarray:
            return self._ids_or_minus_one(values, self._known_user_id, n_users)

        def item_index(values: np.ndarray) -> np.ndarray:
            return self._ids_or_minus_one(values, self.item_ids.get_id, min(n_items, 2 ** 31 - 1))

        users, items = np.asarray(users), np.asarray(items)
        eval_users, rows, tptr, titems, _ = ground_truth_csr(users, items, user_index, item_index)
        in_frame = ~_missing(users)
        held = items[in_frame]
        held = held[~_missing(held)]
        distinct, pos = _distinct(held) if len(held) else (held, np.empty(0, np.int64))
        known_rows = int((item_index(distinct)[pos] >= 0).sum()) if len(held) else 0
        unknown_items = int(in_frame.sum()) - known_rows
        keep = (rows >= 0) & (np.diff(tptr) > 0)
        skipped = int((~keep).sum())
        sel = np.repeat(keep, np.diff(tptr))
        kept_ptr = np.zeros(int(keep.sum()) + 1, dtype=np.int64)
        np.cumsum(np.diff(tptr)[keep], out=kept_ptr[1:])
        above, tied, score, competing = self._catalogue_ranks(rows[keep], kept_ptr, titems[sel].astype(np.int64), filter_interacted)
        return eval_users[keep], kept_ptr, above, tied, score, competing, unknown_items, skipped

    # ------------------------------------------------------------ diversified lists (an extension: the reference has none)
    DIVERSE_MAX_POOL = 1024     # list length rtrec_slim_diversify_lists re-ranks

    @staticmethod
    def _mmr_lambda(diversity: float, what: str) -> np.float32:
        """lambda = float32(1 - diversity) of the greedy selection; a diversity outside [0, 1] (or NaN) is refused."""
        if not 0.0 <= float(diversity) <= 1.0:
            raise ValueError(f"{what}: diversity must lie in [0, 1], got {diversity}")
        return np.float32(1.0 - float(diversity))

    def _diverse_args(self, what: str, top_k: int, pool: int, diversity: float) -> Tuple[int, int, np.float32]:
        """(top_k, pool, lambda) of a diversified call named `what`, or its refusal."""
        top_k, pool = int(top_k), int(pool)
        if not 1 <= top_k <= pool <= self.DIVERSE_MAX_POOL:
            raise ValueError(f"{what} needs 1 <= top_k <= pool <= {self.DIVERSE_MAX_POOL}, got top_k={top_k} and "
                             f"pool={pool}")
        lam = self._mmr_lambda(diversity, what)
        if not self.model.is_fitted:
            raise RuntimeError(f"Model must be fitted before calling {what}.")
        return top_k, pool, lam

    def _pool_width(self, what: str, pool: int, mode: int) -> int:
        """min(pool, the catalogue): the width of the lists the scoring pass of `what` hands to the selection, refused where the
        fused top-k kernels do not serve it for this model (the weights are synced by the caller)."""
        eng = self.model.engine
        k_pool = min(pool, self.model.n_items_fitted)
        if k_pool < 1 or not eng.topk_supported(k_pool, mode):
            why = (f"they rank lists of at most {eng.MAX_TOP_K} items" if k_pool > eng.MAX_TOP_K else
                   f"the per-tile lists of one user, (pool + 1) per tile of W's columns, exceed the {eng.MAX_MERGE_CANDIDATES} "
                   "entries the merge takes") if k_pool >= 1 else "the model has no item"
            raise ValueError(f"{what}: the fused score + top-k kernels do not serve lists of pool={pool} for "
                             f"this model ({why}): choose a smaller pool")
        return k_pool

    def _diverse_device(self, rows: np.ndarray, top_k: int, k_pool: int, lam: float, filter_interacted: bool, mode: int):
        """The device section of the diversified calls for the user rows `rows` (int32, inside the matrix): device tensors
        (ids[n, keep] int32, base scores[n, keep] float32, counts[n] int32, value[n, keep], penalty[n, keep]), keep =
        min(top_k, k_pool); -1 / -inf behind counts.  The scoring kernels' lists of k_pool go straight into the selection
        kernel and the chosen entries are gathered where the lists are, so nothing has left HBM yet."""
        eng = self.model.engine
        torch = eng.be.torch
        d_ids, d_sc, d_cnt = eng.score_topk_device(None, len(rows), k_pool, filter_interacted, mode, d_rows=eng._up(rows))
        d_sc = d_sc.to(torch.float32)
        order, value, pen, cnt = eng.diversify_device(d_ids, d_sc, d_cnt, min(top_k, k_pool), lam)
        gone = order < 0
        at = order.clamp(min=0).to(torch.int64)
        g_ids = torch.gather(d_ids, 1, at).masked_fill(gone, -1)
        g_sc = torch.gather(d_sc, 1, at).masked_fill(gone, float("-inf"))
        return g_ids, g_sc, cnt, value, pen

    def recommend_diverse_batch(self, users: List[Any], top_k: int = 10, pool: int = 50, diversity: float = 0.3,
                                filter_interacted: bool = True, ret_scores: bool = False, as_arrays: bool = False) -> Any:
        """Recommendations that trade score against similarity to what is already on the page: a list ranked by score alone
        tends to be the neighbours of the two or three items the user rated.  Per user the `pool` best items are scored as
        `recommend_batch` scores them, and `top_k` of them are chosen greedily (maximal marginal relevance): every step takes
        the item with the largest lambda * score - (1 - lambda) * penalty, lambda = float32(1 - diversity), penalty = the
        largest similarity to an item already chosen, similarity(a, b) = max(|W[a, b]|, |W[b, a]|) -- W is the item-item
        similarity SLIM learned.  The first item is always the best-scored one; among equal values the better-scored item
        wins.  `diversity=0` returns `recommend_batch`'s lists; 1 ignores the scores after the first item.  Scores and
        similarities are NOT normalised against each other: W's scale is what the fit made it, so choose `diversity` for the
        model at hand.

        For known users this is one device pass: the scoring kernels' lists of `pool` go straight into the selection kernel
        (csrc/diversify.hip; the contract is the comment of rtrec_slim_diversify_lists in include/rtrec_amd_ext.h), the
        chosen entries are gathered on the device and only `top_k` per user are downloaded.  Unknown users get the first
        `top_k` of their cold-start list unchanged (it carries no scores); users outside the matrix follow
        `recommend_batch`'s rules.  With several ranks the scoring pass is the usual collective and every rank computes the
        same lists.

        Raises ValueError unless 1 <= top_k <= pool <= 1024 and 0 <= diversity <= 1; for a pool the fused top-k kernels do not
        serve for this model -- they rank at most 1023 items, so 1024 is served only by a catalogue of fewer items, and a wide
        catalogue lowers the limit further (its per-tile lists must fit the merge); for a W whose values are not float32 numbers (a float64 W holding float32 numbers is served
        with them); and for a column-sharded W (gather it with gather_item_similarity()).

        Returns one list of raw item ids per user -- of (item, base score) tuples with `ret_scores` -- or with
        `as_arrays=True` (ids[B, top_k], scores[B, top_k], counts[B], value[B, top_k], penalty[B, top_k]): what
        `rerank_batch(as_arrays=True)` returns (INTERNAL item ids, base scores, -1 / -inf behind counts[b]) plus the value the
        entry was chosen with and its penalty, i.e. how similar it is to what stands above it (-inf for the unchanged lists
        of unknown users)."""
        top_k, pool, lam = self._diverse_args("recommend_diverse_batch", top_k, pool, diversity)
        batch = self._user_batch(users)
        out_ids, out_sc, out_val, out_pen, out_cnt = self._padded(batch.B, top_k, np.int64, np.float32, np.float32, np.float32)
        if batch.B:                                # (an empty batch syncs nothing and asks nothing of W)
            eng = self.model.engine
            self.model._sync_weights()
            eng._whole_w("diversify")              # a W that cannot be served is refused whatever the batch holds
            mode = self._topk_mode()
            k_pool = self._pool_width("recommend_diverse_batch", pool, mode)
            self._fill_unserved(batch, top_k, filter_interacted, out_ids, out_cnt, out_sc)
            if batch.regular.any():
                self._sync_interactions()
                keep = min(top_k, k_pool)
                g_ids, g_sc, cnt, value, pen = self._diverse_device(batch.uid[batch.regular].astype(np.int32), top_k, k_pool, lam,
                                                                    filter_interacted, mode)
                pos = np.flatnonzero(batch.regular)
                out_ids[pos, :keep], out_sc[pos, :keep] = g_ids.cpu().numpy(), g_sc.cpu().numpy()
                out_val[pos, :keep], out_pen[pos, :keep], out_cnt[pos] = value.cpu().numpy(), pen.cpu().numpy(), cnt.cpu().numpy()
        if as_arrays:
            return out_ids, out_sc, out_cnt, out_val, out_pen
        return self._lists_tail(out_ids, out_cnt, out_sc if ret_scores else None)

    def recommend_diverse(self, user: Any, top_k: int = 10, pool: int = 50, diversity: float = 0.3, filter_interacted: bool = True,
                          ret_scores: bool = False) -> List[Any]:
        """recommend_diverse_batch for one user: the diversified list, or (item, base score) tuples."""
        return self.recommend_diverse_batch([user], top_k=top_k, pool=pool, diversity=diversity, filter_interacted=filter_interacted,
                                            ret_scores=ret_scores)[0]

    def diversify_batch(self, items: List[List[Any]], scores: List[List[float]], top_k: int = 10, diversity: float = 0.3,
                        as_arrays: bool = False) -> Any:
        """The selection of recommend_diverse_batch for lists the caller brings -- from another ranker, a rule, a cache; no
        user is needed: `items` holds one list of raw item ids per row, best first, `scores` their base scores (one per item,
        finite; an entry with a non-finite score does not compete).  An item the model does not know is an empty position, an
        item listed twice is shown once (at its first chosen entry).  Lists longer than 1024 raise ValueError, as do
        `top_k < 1` and a `diversity` outside [0, 1].

        Returns per row the `top_k` chosen (item, base score) tuples in their new order -- or with `as_arrays=True`
        (order[B, keep], value[B, keep], penalty[B, keep], counts[B]), keep = min(top_k, the longest list): order holds list
        POSITIONS, value / penalty the step's value and the entry's similarity to what stands above it, -1 / -inf / -inf
        behind counts[b]."""
        lam = self._mmr_lambda(diversity, "diversify_batch")
        if not self.model.is_fitted:
            raise RuntimeError("Model must be fitted before calling diversify_batch.")
        items, scores = [list(r) for r in items], [list(r) for r in scores]
        if len(items) != len(scores) or any(len(a) != len(b) for a, b in zip(items, scores)):
            raise ValueError("scores must hold one list per list of items, and one score per item")
        K = max([len(r) for r in items] + [1])
        if int(top_k) < 1 or K > self.DIVERSE_MAX_POOL:
            raise ValueError(f"diversify_batch serves top_k >= 1 and lists of up to {self.DIVERSE_MAX_POOL} items, got top_k={top_k} "
                             f"and a list of {K}")
        n_items = self.model.n_items_fitted
        ids = [self._ids_or_minus_one(r, self.item_ids.get_id, min(n_items, 2 ** 31 - 1)).tolist() for r in items]
        order, value, pen, cnt = self.model.diversify_batch(ids, scores, top_k=int(top_k), lam=lam)
        if as_arrays:
            return order, value, pen, cnt
        return [[(items[b][p_], float(scores[b][p_])) for p_ in order[b, :cnt[b]].tolist()] for b in range(len(items))]

    # ------------------------------------------------------------ blended lists (the reference's hybrid merge, on the device)
    BLEND_MAX_LIST = 1024       # list length rtrec_slim_blend_lists takes on either side

    @staticmethod
    def _blend_weight(weighting: Any, what: str) -> Tuple[bool, float]:
        """(contacts, constant weight) of a `weighting` argument: "contacts" or a non-negative number."""
        if isinstance(weighting, str):
            if weighting != "contacts":
                raise ValueError(f'{what}: weighting must be "contacts" or a non-negative number, got {weighting!r}')
            return True, 1.0
        w = float(weighting)
        if not w >= 0.0:                                                  # (a NaN fails the compare)
            raise ValueError(f'{what}: weighting must be "contacts" or a non-negative number, got {weighting!r}')
        return False, w

    @staticmethod
    def _weight_factor(similarity_weight_factor: float, what: str) -> float:
        """The k of the contacts rule weight = 2 n / (n + k), or its refusal."""
        k = float(similarity_weight_factor)
        if not k >= 0.0:                                                  # (a NaN fails the compare)
            raise ValueError(f"{what}: similarity_weight_factor must not be negative or NaN, got {similarity_weight_factor}")
        return k

    def _brought_lists(self, what: str, items: List[List[Any]], scores: List[List[float]], n_rows: Optional[int] = None):
        """(ids[B, K] int32, scores[B, K] float32, counts[B] int32) of the raw-id lists `items` with `scores`: ids the model does
        not know are dropped (with their scores) before upload, so they never cut a list.  Lists of lists, or -- for integer
        ids -- two [B, K] arrays."""
        bound = min(self.model.n_items_fitted, 2 ** 31 - 1)
        if (isinstance(items, np.ndarray) and items.ndim == 2 and items.dtype.kind in "iu" and self.item_ids.pass_through
                and 1 <= items.shape[1] <= self.BLEND_MAX_LIST and np.shape(scores) == items.shape
                and (n_rows is None or items.shape[0] == n_rows)):
            # integer ids that pass through unmapped, as two [B, K] arrays: the same dropping without a Python loop per item
            known = (items >= 0) & (items < bound)
            if known.all():
                return items.astype(np.int32), np.ascontiguousarray(scores, dtype=np.float32), np.full(len(items), items.shape[1], np.int32)
            order = np.argsort(~known, axis=1, kind="stable")           # the known ids to the front, in their order
            ids = np.take_along_axis(np.where(known, items, -1), order, axis=1).astype(np.int32)
            val = np.take_along_axis(np.where(known, np.asarray(scores, dtype=np.float32), np.float32(0.0)), order, axis=1)
            return ids, val, known.sum(axis=1).astype(np.int32)
        items, scores = [list(r) for r in items], [list(r) for r in scores]
        if len(items) != len(scores) or any(len(a) != len(b) for a, b in zip(items, scores)):
            raise ValueError(f"{what}: scores must hold one list per list of items, and one score per item")
        if n_rows is not None and len(items) != n_rows:
            raise ValueError(f"{what}: one list of items is needed per user, got {len(items)} for {n_rows} users")
        if max([len(r) for r in items] + [0]) > self.BLEND_MAX_LIST:
            raise ValueError(f"{what} serves lists of up to {self.BLEND_MAX_LIST} items, got a list of {max(len(r) for r in items)}")
        kept = []
        for r, sc in zip(items, scores):
            iid = self._ids_or_minus_one(r, self.item_ids.get_id, bound)
            known = iid >= 0
            kept.append((iid[known], np.asarray(sc, dtype=np.float32).reshape(-1)[known]))
        K = max([len(i) for i, _ in kept] + [1])
        ids = np.full((len(kept), K), -1, dtype=np.int32)
        val = np.zeros((len(kept), K), dtype=np.float32)
        for b, (i, v) in enumerate(kept):
            ids[b, :len(i)], val[b, :len(i)] = i, v
        return ids, val, np.array([len(i) for i, _ in kept], dtype=np.int32)

    def _contact_csr(self, contact_counts: Optional[Iterable[Tuple[Any, Any, int]]], n_rows: int):
        """The count CSR of rtrec_slim_blend_lists over the `n_rows` rows of X from (user, item, count) triples in raw ids:
        (ptr, col, val) int32 arrays, or None without triples.  Unknown users and items are skipped; a pair given twice keeps
        its last count."""
        if contact_counts is None:
            return None
        n_items = self.model.n_items_fitted
        last = {}
        for user, item, n in contact_counts:
            u = self._ids_or_minus_one([user], self._known_user_id, n_rows)[0]
            i = self._ids_or_minus_one([item], self.item_ids.get_id, n_items)[0]
            if u >= 0 and i >= 0:
                last[(int(u), int(i))] = int(n)
        keys = sorted(last)
        ptr = np.zeros(n_rows + 1, dtype=np.int64)
        for u, _ in keys:
            ptr[u + 1] += 1
        return (np.cumsum(ptr).astype(np.int32), np.array([i for _, i in keys], dtype=np.int32),
                np.clip(np.array([last[key] for key in keys], dtype=np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32))

    def _slim_pool_device(self, rows: np.ndarray, regular: np.ndarray, k_pool: int, filter_interacted: bool, mode: int):
        """SLIM's side of a blend as device tensors (ids[B, k_pool] int32, scores float32, counts[B] int32): the scoring kernels'
        lists for the user rows `rows` where `regular`, empty lists for the others (users without a row)."""
        eng = self.model.engine
        torch = eng.be.torch
        B = len(rows)
        pos = np.flatnonzero(regular)
        if len(pos) == B:                          # SLIM's lists go from the scoring kernels into the blend kernel as they are
            b_ids, b_sc, b_cnt = eng.score_topk_device(None, B, k_pool, filter_interacted, mode, d_rows=eng._up(rows))
            return b_ids, b_sc.to(torch.float32), b_cnt
        b_ids = eng.be.zeros((B, k_pool), torch.int32)
        b_sc = eng.be.zeros((B, k_pool), torch.float32)
        b_cnt = eng.be.zeros((B,), torch.int32)
        if len(pos):
            i, s_, c = eng.score_topk_device(None, len(pos), k_pool, filter_interacted, mode, d_rows=eng._up(rows[pos]))
            at = eng._up(pos.astype(np.int64))
            b_ids[at], b_sc[at], b_cnt[at] = i, s_.to(torch.float32), c
        return b_ids, b_sc, b_cnt

    def recommend_blended_batch(self, users: List[Any], other_items: List[List[Any]], other_scores: List[List[float]], top_k: int = 10,
                                pool: Optional[int] = None, weighting: Any = "contacts",
                                contact_counts: Optional[Iterable[Tuple[Any, Any, int]]] = None, similarity_weight_factor: float = 2.0,
                                mnz: bool = False, filter_interacted: bool = True, as_arrays: bool = False) -> Any:
        """SLIM's list blended with the list of a second scorer -- a factor model, a popularity prior, an editorial ranking --
        the way the reference's hybrid model merges its two halves (HybridSlimFM._ensemble_by_scores): both lists are min-max
        normalised, SLIM's part is weighted per item, the union by item id is sorted by the summed value (the earlier entry
        first among equal values: the other scorer's items in their order, then SLIM's) and cut to `top_k`.

        `other_items` / `other_scores` hold one list per user in raw item ids, best first, with one score per item; ids the
        model does not know are dropped.  SLIM's side is its own top-`pool` list (`pool` defaults to `top_k`, as in the
        reference), scored as `recommend_batch` scores it; unknown users have an empty SLIM side, so their list is the other
        scorer's.  `weighting="contacts"` is the reference's rule: weight = 2 n / (n + similarity_weight_factor), n = how often
        the user touched the item: the count `contact_counts` -- an iterable of (user, item, count) in raw ids, unknown ids
        skipped -- gives for the pair, else 1 for an item the user's row stores and 0 for any other (so with
        `filter_interacted` and no counts SLIM's items weigh nothing, as in the reference).  A non-negative number is a constant
        weight instead.  `mnz=True` doubles the value of an item both lists hold (CombMNZ on the normalised scores).

        For known users this is one device pass: the scoring kernels' lists go straight into the blend kernel (csrc/blend.hip;
        the contract is the comment of rtrec_slim_blend_lists in include/rtrec_amd_ext.h) and only `top_k` per user are
        downloaded.  With several ranks the scoring pass is the usual collective and every rank computes the same lists.

        Raises ValueError unless 1 <= top_k and 1 <= pool <= 1024 and no brought list is longer than 1024; for a `pool` the fused
        top-k kernels do not serve for this model; for a W whose values are not float32 numbers (a float64 W holding float32
        numbers is served with its float32 scores); and for a column-sharded W (gather it with gather_item_similarity()).

        Returns one list of raw item ids per user, or with `as_arrays=True` (ids[B, top_k] int64 INTERNAL item ids,
        value[B, top_k] float32, source[B, top_k] int32 -- 1: only the other scorer holds the item, 2: only SLIM, 3: both --
        counts[B]); -1 / -inf / 0 behind counts[b]."""
        what = "recommend_blended_batch"
        top_k = int(top_k)
        pool = top_k if pool is None else int(pool)
        if top_k < 1 or not 1 <= pool <= self.BLEND_MAX_LIST:
            raise ValueError(f"{what} needs top_k >= 1 and 1 <= pool <= {self.BLEND_MAX_LIST}, got top_k={top_k} and pool={pool}")
        contacts, weight = self._blend_weight(weighting, what)
        k = self._weight_factor(similarity_weight_factor, what)
        self._require_fitted(what)
        users = self._user_list(users)
        B = len(users)
        a_ids, a_sc, a_cnt = self._brought_lists(what, other_items, other_scores, B)      # (refused before the users are looked up)
        out_ids, out_val, out_src, out_cnt = self._padded(B, top_k, np.int64, np.float32, np.int32)
        if B:                                      # (an empty batch syncs nothing and asks nothing of W)
            eng = self.model.engine
            batch = self._user_batch(users)
            self.model._sync_weights()
            eng._whole_w("blend")                  # a W that cannot be served is refused whatever the batch holds
            mode = self._topk_mode()
            k_pool = self._pool_width(what, pool, mode)
            self._sync_interactions()
            rows = batch.rows                      # (a user without a row has an empty SLIM side: no list is filled in)
            b_ids, b_sc, b_cnt = self._slim_pool_device(rows, batch.regular, k_pool, filter_interacted, mode)
            cn = self._contact_csr(contact_counts, eng.n_users) if contacts else None      # (one row per row of the resident X)
            keep = min(top_k, a_ids.shape[1] + k_pool)
            ids, value, source, count = eng.blend_device(eng._up(a_ids), eng._up(a_sc), eng._up(a_cnt), b_ids, b_sc, b_cnt, keep, weight,
                                                         contacts, k, mnz, d_rows=eng._up(rows),
                                                         cn=None if cn is None else tuple(eng._up(a) for a in cn))
            out_ids[:, :keep], out_val[:, :keep] = ids.cpu().numpy(), value.cpu().numpy()
            out_src[:, :keep], out_cnt[:] = source.cpu().numpy(), count.cpu().numpy()
        if as_arrays:
            return out_ids, out_val, out_src, out_cnt
        return self._lists_tail(out_ids, out_cnt)

    def recommend_blended(self, user: Any, other_items: List[Any], other_scores: List[float], top_k: int = 10, pool: Optional[int] = None,
                          weighting: Any = "contacts", contact_counts: Optional[Iterable[Tuple[Any, Any, int]]] = None,
                          similarity_weight_factor: float = 2.0, mnz: bool = False, filter_interacted: bool = True) -> List[Any]:
        """recommend_blended_batch for one user and one brought list."""
        return self.recommend_blended_batch([user], [other_items], [other_scores], top_k=top_k, pool=pool, weighting=weighting,
                                            contact_counts=contact_counts, similarity_weight_factor=similarity_weight_factor, mnz=mnz,
                                            filter_interacted=filter_interacted)[0]

    def blend_batch(self, items_a: List[List[Any]], scores_a: List[List[float]], items_b: List[List[Any]], scores_b: List[List[float]],
                    top_k: int = 10, weight: float = 1.0, mnz: bool = False) -> List[List[Tuple[Any, float]]]:
        """The blend of recommend_blended_batch for two lists the caller brings per row -- no user is needed, so list B is
        weighted by the constant `weight` (non-negative): both lists min-max normalised, united by item id (A's items in their
        order, then the items only B holds), `weight` x B's normalised score added to A's, `mnz` doubling what both hold.  Ids
        the model does not know are dropped.  Returns per row the `top_k` best (item, value) tuples.  Lists longer than 1024,
        `top_k < 1` and a negative or NaN `weight` raise ValueError."""
        what = "blend_batch"
        contacts, w = self._blend_weight(weight, what)
        if contacts or int(top_k) < 1:
            raise ValueError(f"{what} takes a constant non-negative weight and top_k >= 1, got weight={weight!r} and top_k={top_k}")
        self._require_fitted(what)
        A = self._brought_lists(what, items_a, scores_a)
        Bl = self._brought_lists(what, items_b, scores_b, len(A[0]))
        if not len(A[0]):
            return []
        self.model._sync_weights()
        keep = min(int(top_k), A[0].shape[1] + Bl[0].shape[1])
        ids, value, _, count = self.model.engine.blend_lists(A[0], A[1], Bl[0], Bl[1], A[2], Bl[2], keep=keep, weight_b=w, mnz=mnz)
        return self._lists_tail(ids, count, value)

    # ------------------------------------------------------------ factor scorer and hybrid lists (the reference's hybrid, one pass)
    FACTOR_MAX_K = 128          # list length rtrec_factor_topk selects

    def attach_factors(self, users: Iterable[Any], user_vectors: Any, items: Iterable[Any], item_vectors: Any) -> "SLIM":
        """Bring the vectors of a factor model somebody else trained (an exported LightFM or ALS model, an item2vec table, any
        embedding): `user_vectors` [len(users), dim] and `item_vectors` [len(items), dim] for the raw ids `users` / `items`;
        biases are components the caller stacks (utils/factors.stack_bias).  Ids the model does not know are dropped (an id
        given twice keeps its last vector); a known user without a vector gets an empty factor list, a known item without a
        vector is never listed by the factor scorer.  Values that are not float32 numbers are refused.  The vectors are
        uploaded on first use and travel with a pickle of the model."""
        from ..engine import SlimEngine
        users, items = list(users), list(items)
        P = SlimEngine._as_float32(user_vectors, "user_vectors")
        Q = SlimEngine._as_float32(item_vectors, "item_vectors")
        if P.ndim != 2 or Q.ndim != 2 or P.shape[1] != Q.shape[1] or P.shape[0] != len(users) or Q.shape[0] != len(items):
            raise ValueError(f"attach_factors needs one vector per id and one width on both sides, got {P.shape} for {len(users)} "
                             f"users and {Q.shape} for {len(items)} items")
        if not 1 <= P.shape[1] <= SlimEngine.FACTOR_MAX_DIM:
            raise ValueError(f"factor vectors of 1..{SlimEngine.FACTOR_MAX_DIM} components are supported, got {P.shape[1]}")
        uid = self._ids_or_minus_one(users, self._known_user_id)
        iid = self._ids_or_minus_one(items, self.item_ids.get_id)
        self._factors = {"user_rows": uid[uid >= 0], "user_vectors": np.ascontiguousarray(P[uid >= 0]),
                         "item_rows": iid[iid >= 0], "item_vectors": np.ascontiguousarray(Q[iid >= 0])}
        self._factors_on_device = None
        return self

    FACTOR_TRAIN_MAX_DIM = 64   # dim limit of rtrec_factor_als_solve (the default solver)
    FACTOR_TRAIN_CG_MAX_DIM = 256   # dim limit of rtrec_factor_als_cg (solver="cg")

    @classmethod
    def _factor_solver_check(cls, what: str, dim: int, solver: str, cg_steps: int) -> None:
        if solver not in ("cholesky", "cg"):
            raise ValueError(f"{what}: solver must be 'cholesky' or 'cg', got {solver!r}")
        if solver == "cg" and not 1 <= int(dim) <= cls.FACTOR_TRAIN_CG_MAX_DIM:
            raise ValueError(f"{what} solves vectors of 1..{cls.FACTOR_TRAIN_CG_MAX_DIM} components with solver='cg', got {dim}")
        if solver == "cg" and not 1 <= int(cg_steps) <= 64:
            raise ValueError(f"{what}: cg_steps must lie in 1..64, got {cg_steps}")

    def _take_trained_factors(self, eng: Any) -> None:
        """The engine's training state as the vectors attach_factors() would have kept: one row per user / item whose last
        solve ended with status 0, in ascending internal id."""
        P, su, Q, si = eng.als_vectors()
        urows, irows = np.flatnonzero(su == 0).astype(np.int64), np.flatnonzero(si == 0).astype(np.int64)
        self._factors = {"user_rows": urows, "user_vectors": np.ascontiguousarray(P[urows]),
                         "item_rows": irows, "item_vectors": np.ascontiguousarray(Q[irows])}
        eng.als_install()
        n_users, n_items = eng.n_users, self.model.n_items_fitted
        if eng.has_factors() and eng._F["n_items"] == n_items:      # what _sync_factors would upload is resident already
            self._factors_on_device = ((id(self._factors), n_users, n_items, id(eng)), su == 0)
        else:
            self._factors_on_device = None

    def fit_factors(self, dim: int = 32, iterations: int = 15, regularization: float = 0.01, alpha: float = 1.0,
                    seed: int = 0, *, solver: str = "cholesky", cg_steps: int = 3) -> "SLIM":
        """Train the second scorer of the hybrid on the device, from the interactions this model holds: implicit-feedback
        alternating least squares (Hu, Koren, Volinsky) with confidence 1 + alpha * r over the stored, positive interactions,
        `iterations` times a user half-step and an item half-step, deterministic for a `seed` (SlimEngine.fit_factors; the
        pinned arithmetic is the contract of rtrec_factor_gram / rtrec_factor_als_solve in include/rtrec_amd_ext.h).  The
        reference's hybrid trains LightFM there; this is ALS and learns one vector per user and item -- tags still need
        attach_feature_factors().  Leaves the model as attach_factors(users, P, items, Q) with the trained vectors would: a
        user or item without a positive interaction has no vector.  `solver="cholesky"` (the default) solves every row's system
        exactly and trains up to 64 components; `solver="cg"` runs `cg_steps` (1..64) conjugate-gradient steps per row and
        half-step, warm-started from the row's last vector, as `implicit` does by default, and trains up to 256 components
        (rtrec_factor_als_cg).  Returns self."""
        self._factor_solver_check("fit_factors", dim, solver, cg_steps)
        if solver == "cholesky" and not 1 <= int(dim) <= self.FACTOR_TRAIN_MAX_DIM:
            raise ValueError(f"fit_factors trains vectors of 1..{self.FACTOR_TRAIN_MAX_DIM} components, got {dim}")
        if int(iterations) < 1 or not float(regularization) >= 0.0 or not float(alpha) > 0.0:
            raise ValueError(f"fit_factors needs iterations >= 1, regularization >= 0 and alpha > 0, got {iterations}, "
                             f"{regularization} and {alpha}")
        self._sync_interactions_csc()
        eng = self.model.engine
        eng.fit_factors(dim=int(dim), iterations=int(iterations), regularization=float(regularization), alpha=float(alpha), seed=seed,
                        solver=solver, cg_steps=int(cg_steps))
        self._factor_training = {"regularization": float(regularization), "alpha": float(alpha)}
        if solver != "cholesky":                 # (a dict without a solver means Cholesky: an old pickle, attach_factors)
            self._factor_training.update(solver=solver, cg_steps=int(cg_steps))
        self._take_trained_factors(eng)
        return self

    def update_factors(self, users: Iterable[Any], *, solver: Optional[str] = None, cg_steps: Optional[int] = None) -> "SLIM":
        """The online counterpart of fit_factors, to be called after fit / partial_fit of new interactions: the rows of the named
        users are solved again against the current item vectors (one Gram matrix, one solve over a job list), with the
        regularization and alpha of the last fit_factors (its defaults after attach_factors or a pickle).  A user X knows
        and the vectors do not yet gets one; users the model does not know are ignored; item vectors are not touched (an
        item without one is skipped in every row).  `solver` / `cg_steps` default to those of the last fit_factors (Cholesky
        after attach_factors); `solver="cg"` re-solves vectors of up to 256 components, each warm-started from the user's
        present vector.  RuntimeError without fitted or attached vectors."""
        if self._factors is None:
            raise RuntimeError("fit_factors() or attach_factors() must be called before update_factors.")
        if self.has_feature_factors():
            raise ValueError("update_factors solves one vector per user; attach_feature_factors() brought per-feature tables")
        F = self._factors
        dim = int(F["user_vectors"].shape[1])
        par = getattr(self, "_factor_training", None) or {"regularization": 0.01, "alpha": 1.0}
        solver = par.get("solver", "cholesky") if solver is None else solver
        cg_steps = par.get("cg_steps", 3) if cg_steps is None else cg_steps
        self._factor_solver_check("update_factors", dim, solver, cg_steps)
        if solver == "cholesky" and dim > self.FACTOR_TRAIN_MAX_DIM:
            raise ValueError(f"update_factors solves vectors of 1..{self.FACTOR_TRAIN_MAX_DIM} components, the attached ones have {dim}")
        self._sync_interactions_csc()
        eng = self.model.engine
        n_users, n_items = eng.n_users, eng.n_items
        rows = self._ids_or_minus_one(list(users), self._known_user_id, n_users)
        rows = np.unique(rows[rows >= 0])
        P, su = np.zeros((n_users, dim), np.float32), np.ones(n_users, np.uint8)
        ok = F["user_rows"] < n_users
        P[F["user_rows"][ok]], su[F["user_rows"][ok]] = F["user_vectors"][ok], 0
        Q, si = np.zeros((n_items, dim), np.float32), np.ones(n_items, np.uint8)
        ok = F["item_rows"] < n_items
        Q[F["item_rows"][ok]], si[F["item_rows"][ok]] = F["item_vectors"][ok], 0
        eng.als_begin(dim, par["regularization"], par["alpha"], Q, user_vectors=P, user_status=su, item_status=si, solver=solver,
                      cg_steps=int(cg_steps))
        if len(rows):
            eng.als_half_step("user", rows)
        self._take_trained_factors(eng)
        return self

    def attach_feature_factors(self, users: Iterable[Any], user_tags: Iterable[Any], user_table: Any, items: Iterable[Any],
                               item_tags: Iterable[Any], item_table: Any, user_bias: Any = None, item_bias: Any = None) -> "SLIM":
        """Bring the per-FEATURE tables of a factor model trained with feature rows (an exported LightFM model trained the
        reference's way: `model.user_embeddings` / `model.user_biases` go in as they are): `user_table`
        [len(users) + len(user_tags), dim_e] holds first the identity rows of the raw ids `users`, then the rows of the tag
        strings `user_tags`; `item_table` the same for `items` / `item_tags`; `user_bias` / `item_bias` (one entry per table
        row) go in on both sides or on neither.  Where attach_factors() wants one finished vector per id, the vector of an
        entity is computed here, on the device (csrc/feature_repr.hip): its feature row -- the identity column, then the
        columns of its tags (utils/factors.feature_rows) -- times the table, stacked [b, 1, e...] / [1, b, e...] as the
        reference stacks biases.  The tags are those registered with register_user_feature / register_item_feature; a tag
        registered or cleared later is seen by the next call.  `users_tags` of recommend_factor_batch /
        recommend_hybrid_batch replace a user's registered tags for one call and give an unknown user a vector of its own.
        Ids the model does not know are dropped (their table rows are never read); a tag the table does not know is
        skipped.  Values that are not float32 numbers are refused.  Travels with a pickle of the model; detach_factors()
        clears it."""
        from ..engine import SlimEngine
        users, items, user_tags, item_tags = list(users), list(items), list(user_tags), list(item_tags)
        if (user_bias is None) != (item_bias is None):
            raise ValueError("attach_feature_factors takes biases on both sides or on neither: the stacked vectors pair a bias "
                             "with a constant 1 on the other side")
        tables = {}
        for side, ids, tags, table, bias in (("user", users, user_tags, user_table, user_bias), ("item", items, item_tags, item_table, item_bias)):
            E = SlimEngine._as_float32(table, f"{side}_table")
            if E.ndim != 2 or E.shape[0] != len(ids) + len(tags):
                raise ValueError(f"{side}_table needs one row per id and then one per tag ({len(ids)} + {len(tags)}), got {E.shape}")
            b = None
            if bias is not None:
                b = SlimEngine._as_float32(bias, f"{side}_bias").reshape(-1)
                if b.shape[0] != E.shape[0]:
                    raise ValueError(f"{side}_bias needs one entry per row of {side}_table ({E.shape[0]}), got {b.shape[0]}")
            tables[side] = (E, b)
        dim_e = tables["user"][0].shape[1]
        if tables["item"][0].shape[1] != dim_e:
            raise ValueError(f"user_table and item_table must have one width, got {tables['user'][0].shape} and {tables['item'][0].shape}")
        dim = dim_e + (2 if user_bias is not None else 0)
        if dim_e < 1 or dim > SlimEngine.FACTOR_MAX_DIM:
            raise ValueError(f"factor vectors of 1..{SlimEngine.FACTOR_MAX_DIM} components are supported (the two bias slots "
                             f"included), got {dim}")
        uid = self._ids_or_minus_one(users, self._known_user_id)
        iid = self._ids_or_minus_one(items, self.item_ids.get_id)
        self._factors = {"kind": "features",
                         "user_rows": uid[uid >= 0], "user_cols": np.flatnonzero(uid >= 0), "user_tags": user_tags,
                         "user_table": tables["user"][0], "user_bias": tables["user"][1],
                         "item_rows": iid[iid >= 0], "item_cols": np.flatnonzero(iid >= 0), "item_tags": item_tags,
                         "item_table": tables["item"][0], "item_bias": tables["item"][1]}
        self._factors_on_device = None
        return self

    def has_feature_factors(self) -> bool:
        return self._factors is not None and self._factors.get("kind") == "features"

    def _feature_rows_of(self, side: str, ids: np.ndarray, tags: Optional[List[Any]] = None):
        """The feature rows (utils/factors.feature_rows) of the internal ids `ids` of `side` ("user" / "item"; a negative id:
        an entity without an identity, a cold user) against the attached table: with `tags` None the tags registered in the
        feature store, else one tag list per id that REPLACES them."""
        from ..utils.factors import feature_rows
        F = self._factors
        n_ids = int(F[f"{side}_table"].shape[0]) - len(F[f"{side}_tags"])
        tag_cols = {t: n_ids + j for j, t in enumerate(F[f"{side}_tags"])}
        ids = np.asarray(ids, dtype=np.int64)
        rows, cols = F[f"{side}_rows"], F[f"{side}_cols"]
        ident_of = np.full(max(int(rows.max()) + 1 if len(rows) else 0, int(ids.max()) + 1 if len(ids) else 0, 1), -1, dtype=np.int64)
        ident_of[rows] = cols
        ident = np.where(ids >= 0, ident_of[np.maximum(ids, 0)], -1)
        if tags is None:
            store = self.feature_store._users if side == "user" else self.feature_store._items
            vocab, by_entity = store.vocab, store.by_entity
            tags = [[vocab[f] for f in by_entity.get(int(e), ())] if by_entity else () for e in ids]
        return feature_rows(ident, tags, tag_cols, int(F[f"{side}_table"].shape[0]))

    def detach_factors(self) -> "SLIM":
        self._factors = None
        self._factors_on_device = None
        if self.model._engine is not None:
            self.model._engine.clear_factors()
        return self

    def has_factors(self) -> bool:
        return self._factors is not None

    def _sync_factors(self, what: str) -> np.ndarray:
        """Make the engine's resident vectors current for the resident X and W (interactions synced by the caller); returns the
        bool array over X's rows: this row has a vector."""
        if self._factors is None:
            raise RuntimeError(f"attach_factors() must be called before {what}.")
        eng, F = self.model.engine, self._factors
        n_users, n_items = eng.n_users, self.model.n_items_fitted
        if F.get("kind") == "features":
            # the vectors are computed on the device from the tables and the registered tags: a tag registered or cleared
            # since (FeatureStore.version) makes them stale, as the reference rebuilds its feature matrices per call
            stamp = (id(F), n_users, n_items, id(eng), id(self.feature_store), self.feature_store.version)
            if self._factors_on_device is None or self._factors_on_device[0] != stamp or not eng.has_factors():
                eng.set_feature_factors(self._feature_rows_of("user", np.arange(n_users)), F["user_table"],
                                        self._feature_rows_of("item", np.arange(n_items)), F["item_table"],
                                        user_bias=F["user_bias"], item_bias=F["item_bias"])
                self._factors_on_device = (stamp, eng._F["index"].cpu().numpy() >= 0)
            return self._factors_on_device[1]
        stamp = (id(F), n_users, n_items, id(eng))
        if self._factors_on_device is None or self._factors_on_device[0] != stamp or not eng.has_factors():
            dim = F["user_vectors"].shape[1]
            index = np.full(n_users, -1, dtype=np.int64)
            ok = F["user_rows"] < n_users
            index[F["user_rows"][ok]] = np.flatnonzero(ok)
            Q = np.zeros((n_items, dim), dtype=np.float32)
            mask = np.zeros(n_items, dtype=np.uint8)
            ok = F["item_rows"] < n_items
            Q[F["item_rows"][ok]] = F["item_vectors"][ok]
            mask[F["item_rows"][ok]] = 1
            eng.set_factors(F["user_vectors"], Q, user_index=index, item_mask=mask)
            self._factors_on_device = (stamp, index >= 0)
        return self._factors_on_device[1]

    def _checked_users_tags(self, what: str, users: Any, users_tags: Any) -> Optional[List[List[Any]]]:
        """`users_tags` of a recommend_factor / recommend_hybrid call as one list of tags per user, or None."""
        if users_tags is None:
            return None
        if not self.has_feature_factors():
            why = ("no factor model is attached" if self._factors is None else
                   "attach_factors() brought one finished vector per id, which a tag cannot change")
            raise ValueError(f"{what}: users_tags needs the per-feature tables of attach_feature_factors(): {why}")
        if any(isinstance(t, (str, bytes)) for t in users_tags):
            raise ValueError(f"{what}: users_tags holds one LIST of tags per user, got a string")
        users_tags = [[] if t is None else list(t) for t in users_tags]
        if len(users_tags) != len(users):
            raise ValueError(f"{what}: users_tags must hold one list of tags per user, got {len(users_tags)} lists for {len(users)} users")
        return users_tags

    def _brought_user_vectors(self, uid: np.ndarray, regular: np.ndarray, users_tags: List[List[Any]]):
        """The vectors of one call with `users_tags` (device tensors: vectors[B, dim], has[B] uint8): a known user's identity
        column plus the tags of the call (its registered tags are replaced, as in the reference's _recommend_hot_batch), an
        unknown user's tags alone (_cold_user_features)."""
        rows = self._feature_rows_of("user", np.where(regular, uid, -1), users_tags)
        return self.model.engine.feature_vectors_device(rows, "user")

    def recommend_factor_batch(self, users: List[Any], top_k: int = 10, filter_interacted: bool = True,
                               candidate_items: Optional[List[Any]] = None, as_arrays: bool = False,
                               users_tags: Optional[List[List[Any]]] = None) -> Any:
        """The second scorer alone: per user the `top_k` items by the dot product of the attached user and item vectors (the
        reference's implicit.topk call of its hybrid model) -- a float32 fused multiply-add chain over ascending components,
        the larger score first, the lower internal item id among equal scores -- among the items that have a vector, that
        `candidate_items` (raw ids, unknown ones dropped; None: all) names and, with `filter_interacted`, that the user has
        not touched.  One device pass (csrc/factor_topk.hip; the contract is the comment of rtrec_factor_topk in
        include/rtrec_amd_ext.h).  An unknown user, a user outside the matrix and a user without a vector get the cold-start
        list `recommend_batch` gives unknown users (scores 0).  Raises ValueError unless 1 <= top_k <= 128.

        `users_tags` (attach_feature_factors() only; ValueError otherwise): one list of tag strings per user that REPLACES
        the user's registered tags for this call (an empty list: the identity alone), as in the reference.  An unknown user
        whose tags the table knows gets the list of its tag-only vector over the catalogue (or `candidate_items`), nothing
        filtered, scores as computed: the reference's cold start.  An unknown user without such a tag gets the cold-start
        list as before.

        Returns one list of raw item ids per user, or with `as_arrays=True` (ids[B, top_k] int64 INTERNAL item ids,
        scores[B, top_k] float32, counts[B]); -1 / -inf behind counts[b]."""
        what = "recommend_factor_batch"
        top_k = int(top_k)
        if not 1 <= top_k <= self.FACTOR_MAX_K:
            raise ValueError(f"{what} needs 1 <= top_k <= {self.FACTOR_MAX_K} (what the factor kernel selects), got {top_k}")
        users_tags = self._checked_users_tags(what, users, users_tags)
        self._require_fitted(what)
        if self._factors is None:
            raise RuntimeError(f"attach_factors() must be called before {what}.")
        batch = self._user_batch(users)
        B, uid, regular = batch.B, batch.uid, batch.regular
        out_ids, out_sc, out_cnt = self._padded(B, top_k, np.int64, np.float32)
        if B:
            eng = self.model.engine
            n_items = self.model.n_items_fitted
            self.model._sync_weights()
            self._sync_interactions()
            has_vec = self._sync_factors(what)
            vec = None
            if users_tags is not None:
                vec, d_has = self._brought_user_vectors(uid, regular, users_tags)
                served = d_has.cpu().numpy() != 0
            else:
                served = regular.copy()
                served[regular] = has_vec[uid[regular]]
            cand = None
            if candidate_items is not None:
                cand = self._ids_or_minus_one(candidate_items, self.item_ids.get_id, n_items)
                cand = np.unique(cand[cand >= 0])
            # whoever the factor pass does not serve -- no row, or a row without a vector -- gets the cold-start list
            self._fill_unserved(batch, top_k, filter_interacted, out_ids, out_cnt, out_sc,
                                cold_candidates=None if cand is None else cand.tolist(), unserved=~served)
            if served.any():
                mask = None
                if cand is not None:
                    mask = np.zeros(n_items, dtype=np.uint8)
                    mask[cand] = 1
                pos = np.flatnonzero(served)
                if vec is not None:                           # (a user without a row of X: scored unfiltered, the cold start)
                    at = None if len(pos) == B else eng._up(pos.astype(np.int64))
                    ids, sc, cnt = eng.factor_topk_rows(batch.rows[pos], top_k, filter_interacted, item_mask=mask,
                                                        vectors=vec if at is None else vec.index_select(0, at))
                else:
                    ids, sc, cnt = eng.factor_topk_rows(uid[pos], top_k, filter_interacted, item_mask=mask)
                out_ids[pos], out_sc[pos], out_cnt[pos] = ids, sc, cnt
        if as_arrays:
            return out_ids, out_sc, out_cnt
        return self._lists_tail(out_ids, out_cnt)

    def recommend_factor(self, user: Any, top_k: int = 10, filter_interacted: bool = True,
                         candidate_items: Optional[List[Any]] = None, user_tags: Optional[List[Any]] = None) -> List[Any]:
        """recommend_factor_batch for one user (`user_tags`: this user's list of `users_tags`)."""
        return self.recommend_factor_batch([user], top_k=top_k, filter_interacted=filter_interacted, candidate_items=candidate_items,
                                           users_tags=None if user_tags is None else [user_tags])[0]

    def recommend_hybrid_batch(self, users: List[Any], top_k: int = 10, pool: Optional[int] = None, weighting: Any = "contacts",
                               contact_counts: Optional[Iterable[Tuple[Any, Any, int]]] = None, similarity_weight_factor: float = 2.0,
                               mnz: bool = False, filter_interacted: bool = True, as_arrays: bool = False,
                               users_tags: Optional[List[List[Any]]] = None) -> Any:
        """The reference's hybrid list in one device pass: the factor scorer's top-`pool` (recommend_factor_batch's list, from
        the attached vectors) and SLIM's top-`pool` are blended as `recommend_blended_batch` blends a brought list with SLIM's
        -- both min-max normalised, SLIM's part weighted per item (`weighting`, `contact_counts`, `similarity_weight_factor`,
        `mnz` as there), the union sorted by the summed value, the factor scorer's items first among equal values -- and cut
        to `top_k`.  Factor top-k, SLIM's scoring pass and the blend kernel hand their lists on in HBM; only `top_k` per user
        are downloaded.  `pool` defaults to `top_k`, as in the reference.  An unknown user has no row, so both sides and the
        list are empty; a known user without a vector gets SLIM's side alone.  With several ranks every rank computes the same
        lists (the scoring pass is the usual collective; the factor lists are computed locally, no exchange).

        `users_tags` (attach_feature_factors() only; ValueError otherwise): one list of tag strings per user that REPLACES
        the user's registered tags on the factor side for this call, as in the reference.  An unknown user whose tags the
        table knows gets the factor list of its tag-only vector ALONE -- over the whole catalogue, nothing filtered, cut to
        `top_k`, the scores as computed, source 1: the reference's cold start.

        Raises ValueError unless 1 <= top_k and 1 <= pool <= 128: the factor kernel keeps a user's candidates in LDS and
        selects at most 128 per user (SLIM's side alone would take 1024); and for what `recommend_blended_batch` refuses.

        Returns what `recommend_blended_batch` returns: one list of raw item ids per user, or with `as_arrays=True`
        (ids[B, top_k] int64 INTERNAL item ids, value[B, top_k] float32, source[B, top_k] int32 -- 1: only the factor scorer
        holds the item, 2: only SLIM, 3: both -- counts[B]); -1 / -inf / 0 behind counts[b]."""
        what = "recommend_hybrid_batch"
        top_k = int(top_k)
        pool = top_k if pool is None else int(pool)
        if top_k < 1 or not 1 <= pool <= self.FACTOR_MAX_K:
            raise ValueError(f"{what} needs top_k >= 1 and 1 <= pool <= {self.FACTOR_MAX_K}, got top_k={top_k} and pool={pool}: the "
                             f"factor kernel keeps each user's candidates in LDS and selects at most {self.FACTOR_MAX_K} per user")
        contacts, weight = self._blend_weight(weighting, what)
        k = self._weight_factor(similarity_weight_factor, what)
        users_tags = self._checked_users_tags(what, users, users_tags)
        self._require_fitted(what)
        if self._factors is None:
            raise RuntimeError(f"attach_factors() must be called before {what}.")
        batch = self._user_batch(users)
        B, uid, regular = batch.B, batch.uid, batch.regular
        out_ids, out_val, out_src, out_cnt = self._padded(B, top_k, np.int64, np.float32, np.int32)
        if B:                                      # (an empty batch syncs nothing and asks nothing of W)
            eng = self.model.engine
            self.model._sync_weights()
            eng._whole_w("blend")
            mode = self._topk_mode()
            k_pool = self._pool_width(what, pool, mode)
            self._sync_interactions()
            self._sync_factors(what)
            rows = batch.rows                      # (a user without a row has no side at all: no list is filled in)
            d_rows = eng._up(rows)
            if users_tags is None:
                a_ids, a_sc, a_cnt = eng.factor_topk_device(d_rows, B, k_pool, filter_interacted)     # (row -1: an empty list)
            else:                       # the vectors of this call's tags; a user without a row is scored unfiltered (cold start)
                vec, d_has = self._brought_user_vectors(uid, regular, users_tags)
                a_ids, a_sc, a_cnt = eng.factor_topk_device(rows, B, k_pool, filter_interacted, vectors=vec, vector_has=d_has)
            b_ids, b_sc, b_cnt = self._slim_pool_device(rows, regular, k_pool, filter_interacted, mode)
            cn = self._contact_csr(contact_counts, eng.n_users) if contacts else None
            keep = min(top_k, 2 * k_pool)
            ids, value, source, count = eng.blend_device(a_ids, a_sc, a_cnt, b_ids, b_sc, b_cnt, keep, weight, contacts, k, mnz,
                                                         d_rows=d_rows, cn=None if cn is None else tuple(eng._up(a) for a in cn))
            out_ids[:, :keep], out_val[:, :keep] = ids.cpu().numpy(), value.cpu().numpy()
            out_src[:, :keep], out_cnt[:] = source.cpu().numpy(), count.cpu().numpy()
            if users_tags is not None and not regular.all():
                # an unknown user has no SLIM side: it gets the factor list of its tags alone, scores as computed (the
                # reference's _recommend_cold_batch), not a min-max normalised copy of it
                pos = np.flatnonzero(~regular)
                at = eng._up(pos.astype(np.int64))
                kc = min(keep, k_pool)
                c_ids, c_sc = a_ids.index_select(0, at).cpu().numpy()[:, :kc], a_sc.index_select(0, at).cpu().numpy()[:, :kc]
                c_cnt = np.minimum(a_cnt.index_select(0, at).cpu().numpy(), kc)
                out_ids[pos], out_val[pos], out_src[pos] = -1, -np.inf, 0
                out_ids[pos, :kc], out_val[pos, :kc], out_cnt[pos] = c_ids, c_sc, c_cnt
                out_src[pos, :kc] = (np.arange(kc)[None, :] < c_cnt[:, None]).astype(np.int32)
        if as_arrays:
            return out_ids, out_val, out_src, out_cnt
        return self._lists_tail(out_ids, out_cnt)

    def recommend_hybrid(self, user: Any, top_k: int = 10, pool: Optional[int] = None, weighting: Any = "contacts",
                         contact_counts: Optional[Iterable[Tuple[Any, Any, int]]] = None, similarity_weight_factor: float = 2.0,
                         mnz: bool = False, filter_interacted: bool = True, user_tags: Optional[List[Any]] = None) -> List[Any]:
        """recommend_hybrid_batch for one user (`user_tags`: this user's list of `users_tags`)."""
        return self.recommend_hybrid_batch([user], top_k=top_k, pool=pool, weighting=weighting, contact_counts=contact_counts,
                                           similarity_weight_factor=similarity_weight_factor, mnz=mnz,
                                           filter_interacted=filter_interacted,
                                           users_tags=None if user_tags is None else [user_tags])[0]

    # ------------------------------------------------------------ list quality (an extension: the reference has none)
    QUALITY_MAX_LIST = 1024     # list length rtrec_slim_list_quality measures

    def list_quality_batch(self, items: List[List[Any]], as_arrays: bool = False) -> Any:
        """What each list of `items` (raw item ids; from this model, another ranker, a rule, a cache -- no user is needed)
        looks like apart from its accuracy.  An item the model does not know is not counted, an item listed twice is judged
        once, at its first place.  Per list a dict: `n` the counted items, `intra_list_similarity` the mean of
        similarity(a, b) = max(|W[a, b]|, |W[b, a]|) over its pairs (NaN below two items), `linked_pairs` the pairs with a
        similarity above 0, `novelty` the mean self-information log2(n_users / the item's users) of its items (NaN for no
        item).  The figures come from one kernel over the lists (csrc/list_quality.hip; the contract is the comment of
        rtrec_slim_list_quality in include/rtrec_amd_ext.h) and utils.metrics.list_quality_figures.  With `as_arrays=True`:
        the kernel's raw arrays (n[B], sim_sum[B], linked[B], weight_sum[B]) plus exposure[n_items], how often each INTERNAL
        item id was counted over all lists.  Lists longer than 1024 raise ValueError; W must be whole and hold float32
        numbers, as for recommend_diverse_batch."""
        from ..utils.metrics import quality_frame_columns
        if not self.model.is_fitted:
            raise RuntimeError("Model must be fitted before calling list_quality_batch.")
        items = [list(r) for r in items]
        K = max([len(r) for r in items] + [1])
        if K > self.QUALITY_MAX_LIST:
            raise ValueError(f"list_quality_batch serves lists of up to {self.QUALITY_MAX_LIST} items, got a list of {K}")
        n_items = self.model.n_items_fitted
        ids = np.full((len(items), K), -1, dtype=np.int32)
        for b, row in enumerate(items):
            ids[b, :len(row)] = self._ids_or_minus_one(row, self.item_ids.get_id, min(n_items, 2 ** 31 - 1))
        counts = np.array([len(r) for r in items], dtype=np.int32)
        self.model._sync_weights()
        self.model.engine._whole_w("list_quality")
        self._sync_interactions()
        n, sim_sum, linked, weight_sum, exposure = self.model.engine.list_quality_lists(ids, counts, novelty=True)
        if as_arrays:
            return n, sim_sum, linked, weight_sum, exposure
        cols = {key: col.tolist() for key, col in quality_frame_columns(n, sim_sum, linked, weight_sum).items()}
        return [{key: cols[key][b] for key in cols} for b in range(len(items))]

    def list_quality(self, items: List[Any]) -> Dict[str, Any]:
        """list_quality_batch for one list: {n, intra_list_similarity, linked_pairs, novelty}."""
        return self.list_quality_batch([items])[0]

    def _hot_lists_device(self, rows: np.ndarray, top_k: int, lam: Optional[float], k_pool: int, filter_interacted: bool, mode: int):
        """Device (ids[n, <= top_k] int32, counts[n] int32) of the lists the user rows `rows` are served: recommend_batch's
        (lam None) or recommend_diverse_batch's."""
        if lam is None:
            ids, _, cnt = self.model.engine.score_topk_device(rows.astype(np.int32), len(rows), top_k, filter_interacted, mode,
                                                              with_scores=False)
            return ids, cnt
        ids, _, cnt, _, _ = self._diverse_device(rows.astype(np.int32), top_k, k_pool, lam, filter_interacted, mode)
        return ids, cnt

    def recommend_quality(self, users: List[Any], top_k: int = 10, diversity: float = 0.0, pool: int = 50,
                          filter_interacted: bool = True, per_user: bool = False) -> Any:
        """What the lists these users would be served look like, and what all of them together show of the catalogue: with
        `diversity == 0` the lists of `recommend_batch(users, top_k=top_k)`, otherwise those of
        `recommend_diverse_batch(users, top_k, pool, diversity)` -- so one call per value of `diversity` gives the curve the knob
        is set by.  Known users' lists go from the scoring kernels (through the selection kernel and its gather where asked)
        into the measuring kernel (csrc/list_quality.hip) without leaving HBM; unknown users contribute their cold-start list,
        uploaded once; users outside the matrix follow `recommend_batch`'s rules.  Four numbers per user and one count per
        item are downloaded.

        Returns utils.metrics.quality_summary's dict: n_lists, n_lists_nonempty, n_lists_pairs, mean_length, the means (exactly
        rounded sums, so they do not depend on the order of the users) of intra_list_similarity and linked_share over the
        lists of two items or more and of novelty over the lists of one or more, and distinct_items, coverage (of the
        fitted catalogue) and gini of the exposure.  `per_user=True` returns (dict, frame): n, intra_list_similarity,
        linked_pairs and novelty per user, in the order of `users`.

        Raises what recommend_diverse_batch raises when `diversity > 0`; with `diversity == 0`, `pool` is not read and top_k must
        be one the fused top-k kernels serve for this model."""
        from ..utils.metrics import quality_frame_columns, quality_summary
        what = "recommend_quality"
        lam: Optional[float] = None
        if float(diversity) != 0.0:                                        # (a NaN is not 0: _mmr_lambda refuses it)
            top_k, pool, lam = self._diverse_args(what, top_k, pool, diversity)
        else:
            top_k = int(top_k)
            if not 1 <= top_k <= self.QUALITY_MAX_LIST:
                raise ValueError(f"{what} needs 1 <= top_k <= {self.QUALITY_MAX_LIST}, got top_k={top_k}")
            self._require_fitted(what)
        users = self._user_list(users)
        B = len(users)
        eng = self.model.engine
        n_items = self.model.n_items_fitted
        self.model._sync_weights()                                         # (W and the pool are checked for an empty batch too)
        dw = eng._whole_w("diversify" if lam is not None else "list_quality")
        mode = self._topk_mode()
        k_pool = self._pool_width(what, pool, mode) if lam is not None else 0
        k = min(top_k, n_items)
        if lam is None and (k < 1 or not eng.topk_supported(k, mode)):
            raise ValueError(f"{what}: the fused score + top-k kernels do not serve lists of top_k={top_k} for this model")
        self._sync_interactions()
        be, torch = eng.be, eng.be.torch
        d_ids = torch.full((B, top_k), -1, dtype=torch.int32, device=be.device)
        d_cnt = be.zeros((B,), torch.int32)
        if B:
            batch = self._user_batch(users)
            if batch.regular.any():
                ids, cnt = self._hot_lists_device(batch.uid[batch.regular], k, lam, k_pool, filter_interacted, mode)
                pos = be.to_dev(np.flatnonzero(batch.regular))
                d_ids[pos, :int(ids.shape[1])] = ids
                d_cnt[pos] = cnt
            self._fill_unserved_device(batch, top_k, filter_interacted, d_ids, d_cnt)      # (after the device pass, as its IndexError was)
        exposure = be.zeros((dw.n_items,), torch.int32)
        out = eng.list_quality_device(d_ids, d_cnt, eng.item_novelty_device(), exposure)
        n, sim_sum, linked, weight_sum = (t.cpu().numpy() for t in out)
        summary = quality_summary(n, sim_sum, linked, weight_sum, exposure.cpu().numpy())
        if not per_user:
            return summary
        import pandas as pd
        return summary, pd.DataFrame(quality_frame_columns(n, sim_sum, linked, weight_sum), index=pd.Index(users, name="user"))

    # ------------------------------------------------------------ audience of an item (an extension: the reference has none)
    def _sync_interactions_csc(self) -> None:
        """_sync_interactions, and the CSC orientation of the GPU copy too: the device mirror's, or -- on the branch that
        uploaded the host CSR alone -- one more upload of the store's CSC export (same values, same max_timestamp)."""
        self._sync_interactions()
        eng = self.model.engine
        if not eng.has_csc():
            eng._attach_csc(self.interactions.to_csc())

    def recommend_users_batch(self, items: List[Any], top_n: int = 100, filter_interacted: bool = True,
                              candidate_users: Optional[List[Any]] = None, ret_scores: bool = False,
                              as_arrays: bool = False) -> Any:
        """Which users should be told about an item: per raw item id of `items` the `top_n` (1..1024) users by
        score(u, i) = sum_j X[u, j] * W[j, i], the score `recommend` ranks the pair by -- computed on the X the model serves
        from (decayed to the current max_timestamp) by walking the <= K columns of X that column i of W names
        (csrc/audience.hip).  Eligible are the users with at least one stored term in that sum (the sparse rule: zero and
        negative scores take part), not stored in the item's own column when `filter_interacted`, and in `candidate_users`
        (raw ids; unknown ones are ignored, an empty list leaves nobody) when given.  Among equal scores the user with the
        lower internal id comes first.  An item the model does not know, or one the fit never reached, gets an empty list;
        repeated items are answered independently.  A float64 W whose values are float32 numbers is served with those
        numbers (the float32 model's scores); a W that is not, or a column-sharded one, raises ValueError.

        Returns one list of raw user ids per item -- of (user, score) tuples with `ret_scores` -- or with `as_arrays=True`
        (users[n, top_n], scores[n, top_n], counts[n], eligible[n]): row b is valid up to counts[b], unused slots hold
        -1 / -inf, eligible[b] is the item's reach (it may exceed top_n), and the ids are INTERNAL user ids: for integer ids
        those are the raw ids, for a model with string ids map them with `model.user_ids.get`."""
        if not self.model.is_fitted:
            raise RuntimeError("Model must be fitted before calling recommend_users_batch.")
        items = list(items)
        q = self._ids_or_minus_one(items, self.item_ids.get_id, self.model.n_items_fitted)
        rows = None
        if candidate_users is not None:
            rows = self._ids_or_minus_one(candidate_users, self._known_user_id)
            rows = rows[rows >= 0]
        self.model._sync_weights()
        self.model.engine._audience_check(top_n)  # a W or a top_n that cannot be served is refused before X is touched
        if len(items):
            self._sync_interactions_csc()
        users, scores, counts, eligible = self.model.recommend_users_batch(q, top_n, filter_interacted, rows)
        if as_arrays:
            return users, scores, counts, eligible
        return self._lists_tail(users, counts, scores if ret_scores else None, id_map=self.user_ids)

    def recommend_users(self, item: Any, top_n: int = 100, filter_interacted: bool = True,
                        candidate_users: Optional[List[Any]] = None, ret_scores: bool = False) -> List[Any]:
        """recommend_users_batch for one item: its audience as raw user ids, or (user, score) tuples."""
        return self.recommend_users_batch([item], top_n=top_n, filter_interacted=filter_interacted,
                                          candidate_users=candidate_users, ret_scores=ret_scores)[0]

    def _similar_items(self, query_item_id: int, query_item_tags: Optional[List[str]] = None, top_k: int = 10
                       ) -> List[Tuple[int, float]]:
        return self.model.similar_items(query_item_id, top_k=top_k, ret_ndarrays=False)  # type: ignore

    def _similar_items_batch(self, query_item_ids: List[int], query_item_tags: Optional[List[str]] = None,
                             top_k: int = 10) -> List[List[Tuple[int, float]]]:
        return self.model.similar_items_batch(query_item_ids, top_k=top_k)

    # ------------------------------------------------------------ similar items from the attached vectors, alone and blended with W's
    def _similar_query(self, what: str, query_items: Any, query_items_tags: Any, first_component: Optional[int]):
        """What the two similar_items_* calls share: (internal ids of the queries with -1 for unknown ones, the brought query
        vectors or None, the first component).  Syncs weights, interactions and the resident vectors."""
        if query_items_tags is not None:
            if not self.has_feature_factors():
                why = ("no factor model is attached" if self._factors is None else
                       "attach_factors() brought one finished vector per id, which a tag cannot change")
                raise ValueError(f"{what}: query_items_tags needs the per-feature tables of attach_feature_factors(): {why}")
            if any(isinstance(t, (str, bytes)) for t in query_items_tags):
                raise ValueError(f"{what}: query_items_tags holds one LIST of tags per query item, got a string")
            query_items_tags = [[] if t is None else list(t) for t in query_items_tags]
            if len(query_items_tags) != len(query_items):
                raise ValueError(f"{what}: query_items_tags must hold one list of tags per query item, got {len(query_items_tags)} "
                                 f"lists for {len(query_items)} items")
        if not self.model.is_fitted:
            raise RuntimeError(f"Model must be fitted before calling {what}.")
        if self._factors is None:
            raise RuntimeError(f"attach_factors() must be called before {what}.")
        F = self._factors
        dim = (F["item_table"].shape[1] + (2 if F["item_bias"] is not None else 0)) if self.has_feature_factors() else F["item_vectors"].shape[1]
        if first_component is None:                 # the reference's target matrix: [b, e...] of a stacked [1, b, e...], else all
            first_component = 1 if self.has_feature_factors() and F["item_bias"] is not None else 0
        first_component = int(first_component)
        if not 0 <= first_component < dim:
            raise ValueError(f"{what}: first_component must lie in 0..{dim - 1}, got {first_component}")
        if len(query_items) == 0:
            return np.zeros(0, dtype=np.int64), None, first_component
        if self.model.engine.world_size > 1:
            raise ValueError(f"{what} reads the whole of W and all item vectors on one rank: gather the model with "
                             "gather_item_similarity() and serve similar items from the gathered model")
        n_items = self.model.n_items_fitted
        qid = self._ids_or_minus_one(query_items, self.item_ids.get_id, n_items)
        self.model._sync_weights()
        self._sync_interactions()
        self._sync_factors(what)
        vec = None
        if query_items_tags is not None:          # (a row without an entry the table knows gives the zero vector: an empty factor side)
            vec, _ = self.model.engine.feature_vectors_device(self._feature_rows_of("item", qid, query_items_tags), "item")
        return qid, vec, first_component

    def similar_items_factor_batch(self, query_items: List[Any], top_k: int = 10, query_items_tags: Optional[List[List[Any]]] = None,
                                   first_component: Optional[int] = None, as_arrays: bool = False) -> Any:
        """"More like this" from the attached vectors alone: per query item the `top_k` items by cosine similarity of the item
        vectors -- the factor side of the reference's HybridSlimFM._similar_items: a float32 fused multiply-add chain over
        ascending components, divided by the item's norm (the ranking score), then by the query's; the query itself and the
        items without a vector are never listed; the larger score first, the lower internal id among equal ones.  One device
        pass (csrc/factor_similar.hip; the contract is the comment of rtrec_factor_similar_topk in include/rtrec_amd_ext.h).
        `first_component` selects the components first_component .. dim-1; None is the reference's choice: 1 for feature
        factors attached with biases (the stacked [1, b, e...] becomes [b, e...]), 0 otherwise -- a caller of attach_factors()
        with stack_bias vectors passes 1.  `query_items_tags` (attach_feature_factors() only; ValueError otherwise): one list
        of tag strings per query that REPLACES the item's registered tags for this call; an unknown item whose tags the table
        knows is served from its tag-only vector.  An unknown item without such tags, and an item whose vector is zero, get [].
        Raises ValueError unless 1 <= top_k <= 128, and with more than one rank.

        Returns one list of (raw item id, float) pairs per query, or with `as_arrays=True` (ids[B, top_k] int64 INTERNAL item
        ids, scores[B, top_k] float32, counts[B]); -1 / -inf behind counts[b]."""
        what = "similar_items_factor_batch"
        top_k = int(top_k)
        if not 1 <= top_k <= self.FACTOR_MAX_K:
            raise ValueError(f"{what} needs 1 <= top_k <= {self.FACTOR_MAX_K} (what the factor kernel selects), got {top_k}")
        query_items = list(query_items)
        qid, vec, first = self._similar_query(what, query_items, query_items_tags, first_component)
        B = len(query_items)
        out_ids, out_sc, out_cnt = self._padded(B, top_k, np.int64, np.float32)
        if B:
            ids, sc, cnt, _ = self.model.engine.similar_factor_device(qid, top_k, first, vectors=vec, write_cosine=True)
            out_ids[:], out_sc[:], out_cnt[:] = ids.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()
        if as_arrays:
            return out_ids, out_sc, out_cnt
        return self._lists_tail(out_ids, out_cnt, out_sc)

    def similar_items_factor(self, query_item: Any, top_k: int = 10, query_item_tags: Optional[List[Any]] = None,
                             first_component: Optional[int] = None) -> List[Tuple[Any, float]]:
        """similar_items_factor_batch for one item (`query_item_tags`: this item's list of `query_items_tags`)."""
        return self.similar_items_factor_batch([query_item], top_k=top_k, first_component=first_component,
                                               query_items_tags=None if query_item_tags is None else [query_item_tags])[0]

    def similar_items_hybrid_batch(self, query_items: List[Any], top_k: int = 10, pool: Optional[int] = None,
                                   query_items_tags: Optional[List[List[Any]]] = None, first_component: Optional[int] = None,
                                   as_arrays: bool = False) -> Any:
        """The reference's hybrid similar_items (HybridSlimFM._similar_items) in one device pass: the factor side's top-`pool`
        by cosine (similar_items_factor_batch's list) and the top-`pool` of W's column (similar_items) are each min-max
        normalised in float32 and added per item in FLOAT64, as the reference's comb_sum does; the larger sum first, among equal
        sums the factor side's items in their order, then SLIM's; cut to `top_k`.  The three kernels hand their lists on in HBM
        (csrc/factor_similar.hip, similar_topk, csrc/similar_blend.hip); only `top_k` entries per query are downloaded.  `pool`
        defaults to `top_k`, which is the reference.  `first_component` and `query_items_tags` as in
        similar_items_factor_batch.  Where the reference raises ValueError (min of an empty list) an empty side contributes
        nothing: an item whose column of W is empty gets the factor list alone, an item without a vector SLIM's list alone
        (each normalised), an unknown item with tags the table knows its tag-only factor list, an unknown item without [].
        SLIM.similar_items / similar_items_batch are unchanged: they still return W's column.
        Raises ValueError unless top_k >= 1 and 1 <= pool <= 128; for a column-sharded W or more than one rank (gather the
        model with gather_item_similarity()); and for a W uploaded from float64 values that are not float32 numbers.

        Returns one list of (raw item id, float) pairs per query, or with `as_arrays=True` (ids[B, top_k] int64 INTERNAL item
        ids, value[B, top_k] float64, source[B, top_k] int32 -- 1: only the factor side holds the item, 2: only SLIM, 3: both
        -- counts[B]); -1 / -inf / 0 behind counts[b]."""
        what = "similar_items_hybrid_batch"
        top_k = int(top_k)
        pool = top_k if pool is None else int(pool)
        if top_k < 1 or not 1 <= pool <= self.FACTOR_MAX_K:
            raise ValueError(f"{what} needs top_k >= 1 and 1 <= pool <= {self.FACTOR_MAX_K}, got top_k={top_k} and pool={pool}: the "
                             f"factor kernel keeps each query's candidates in LDS and selects at most {self.FACTOR_MAX_K}")
        query_items = list(query_items)
        qid, vec, first = self._similar_query(what, query_items, query_items_tags, first_component)
        B = len(query_items)
        out_ids, out_val, out_src, out_cnt = self._padded(B, top_k, np.int64, np.float64, np.int32)
        if B:
            keep = min(top_k, 2 * pool)
            ids, value, source, count = self.model.engine.similar_hybrid_device(qid, top_k, pool, first, vectors=vec)
            out_ids[:, :keep], out_val[:, :keep] = ids.cpu().numpy(), value.cpu().numpy()
            out_src[:, :keep], out_cnt[:] = source.cpu().numpy(), count.cpu().numpy()
        if as_arrays:
            return out_ids, out_val, out_src, out_cnt
        return self._lists_tail(out_ids, out_cnt, out_val)

    def similar_items_hybrid(self, query_item: Any, top_k: int = 10, pool: Optional[int] = None,
                             query_item_tags: Optional[List[Any]] = None, first_component: Optional[int] = None
                             ) -> List[Tuple[Any, float]]:
        """similar_items_hybrid_batch for one item (`query_item_tags`: this item's list of `query_items_tags`)."""
        return self.similar_items_hybrid_batch([query_item], top_k=top_k, pool=pool, first_component=first_component,
                                               query_items_tags=None if query_item_tags is None else [query_item_tags])[0]

    # ------------------------------------------------------------ persistence (slim.py:117-149)
    def _serialize(self) -> dict:
        data = {"model": self.model, "interactions": self.interactions, "user_ids": self.user_ids,
                "item_ids": self.item_ids, "feature_store": self.feature_store}
        if self._factors is not None:           # (only when attached: a model without vectors serialises as it always did)
            data["factors"] = self._factors
            if (getattr(self, "_factor_training", None) or {}).get("solver", "cholesky") != "cholesky":
                data["factor_training"] = dict(self._factor_training)      # (only for a solver an old pickle cannot mean)
        return data

    @classmethod
    def _deserialize(cls, data: dict) -> "SLIM":
        instance = cls()
        instance.model = data["model"]
        instance.interactions = data["interactions"]
        instance.user_ids = data["user_ids"]
        instance.item_ids = data["item_ids"]
        instance.feature_store = data["feature_store"]
        instance._factors = data.get("factors")
        instance._factor_training = data.get("factor_training")
        return instance
