"""DataFrame facade: the drop-in for rtrec.recommender.Recommender
(/root/reference/rtrec/recommender.py:20-223).

Same methods, arguments, mini-batching and the same printed wall-clock / "Throughput: N
samples/sec" figure (interactions divided by ingest + fit time, recommender.py:81,126) that
BASELINE.md quotes.  Mini-batches are cut from the DataFrame columns as arrays rather than
through itertuples().
"""
from __future__ import annotations

import math
import time
from typing import Any, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from .models.base import BaseModel
from .utils.metrics import (CATALOGUE_KS, METRIC_COLUMNS, RESULT_KEYS, _query_metrics, catalogue_rank_summary, compute_scores,
                            quality_frame_columns, quality_summary, scores_from_columns)

_COLUMNS = ["user", "item", "tstamp", "rating"]
_COLUMNAR_CHUNK = 1 << 22


class Recommender:
    def __init__(self, model: BaseModel, use_generator: bool = True):
        self.model = model
        self.use_generator = use_generator

    def get_model(self) -> BaseModel:
        return self.model

    def partial_fit(self, user_interactions: Iterable[Tuple[int, int, int, float]],
                    update_interaction: bool = False) -> "Recommender":
        t0 = time.time()
        self.model.fit(user_interactions, update_interaction=update_interaction, progress_bar=False)
        print(f"Fit completed in {time.time() - t0:.2f} seconds")
        return self

    def _register_tags(self, user_tags, item_tags) -> None:
        for user, tags in (user_tags or {}).items():
            self.model.register_user_feature(user, tags)
        for item, tags in (item_tags or {}).items():
            self.model.register_item_feature(item, tags)

    def _ingest_frame(self, train_data: pd.DataFrame, batch_size: int, update_interaction: bool, record: bool,
                      assume_sorted: bool) -> None:
        frame = train_data[_COLUMNS]
        if not assume_sorted:
            frame = frame.sort_values("tstamp", ascending=True)
        columnar = getattr(self.model, "add_interactions_columns", None)
        if columnar is not None and all(frame[c].dtype.kind in "iuf" for c in _COLUMNS):
            # numeric frame: hand the columns over as arrays.  The store applies a chunk with the same
            # sequential semantics as one add_interaction per row, so mini-batch boundaries (batch_size)
            # do not change the result; only the per-row Python objects of the reference loop go away.
            u, i, t, r = (frame[c].to_numpy() for c in _COLUMNS)
            chunk = getattr(self.model, "bulk_chunk_rows", None) or _COLUMNAR_CHUNK
            for s in range(0, len(frame), chunk):
                e = s + chunk
                columnar(u[s:e], i[s:e], t[s:e], r[s:e], update_interaction=update_interaction,
                         record_interactions=record)
            return
        for batch in Recommender.generate_batches(frame, batch_size, as_generator=self.use_generator):
            self.model.add_interactions(batch, update_interaction=update_interaction, record_interactions=record)

    def fit(self, train_data: pd.DataFrame, user_tags: Optional[Dict[Any, List[str]]] = None,
            item_tags: Optional[Dict[Any, List[str]]] = None, batch_size: int = 1_000,
            update_interaction: bool = False, parallel: bool = False, assume_sorted: bool = True) -> "Recommender":
        """Incremental fit: ingest in mini-batches, then refit the items that were touched."""
        t0 = time.time()
        self._register_tags(user_tags, item_tags)
        self._ingest_frame(train_data, batch_size, update_interaction, True, assume_sorted)
        self.model._fit_recorded(parallel=parallel, progress_bar=True)
        dt = time.time() - t0
        print(f"Fit completed in {dt:.2f} seconds")
        print(f"Throughput: {len(train_data) / dt:.2f} samples/sec")
        return self

    def bulk_fit(self, train_data: pd.DataFrame, user_tags: Optional[Dict[Any, List[str]]] = None,
                 item_tags: Optional[Dict[Any, List[str]]] = None, batch_size: int = 1_000,
                 update_interaction: bool = False, parallel: bool = True, assume_sorted: bool = True) -> "Recommender":
        """Ingest everything, then fit every item column."""
        t0 = time.time()
        self._register_tags(user_tags, item_tags)
        self._ingest_frame(train_data, batch_size, update_interaction, False, assume_sorted)
        self.model.bulk_fit(parallel=parallel, progress_bar=True)
        dt = time.time() - t0
        print(f"Fit completed in {dt:.2f} seconds")
        print(f"Throughput: {len(train_data) / dt:.2f} samples/sec")
        return self

    def recommend(self, user: Any, candidate_items: Optional[List[Any]] = None, user_tags: Optional[List[str]] = None,
                  top_k: int = 10, filter_interacted: bool = True) -> List[Any]:
        return self.model.recommend(user, candidate_items, user_tags, top_k, filter_interacted)

    def recommend_batch(self, users: List[Any], candidate_items: Optional[List[Any]] = None,
                        users_tags: Optional[List[List[str]]] = None, top_k: int = 10,
                        filter_interacted: bool = True, as_arrays: bool = False) -> Any:
        """rtrec/recommender.py:141-151.  `as_arrays=True` (extension): (ids[B, top_k], counts[B]) numpy arrays instead of B
        Python lists -- see BaseModel.recommend_batch."""
        if as_arrays:
            return self.model.recommend_batch(users, candidate_items, users_tags, top_k, filter_interacted, as_arrays=True)
        return self.model.recommend_batch(users, candidate_items, users_tags, top_k, filter_interacted)

    def explain(self, user: Any, items: Optional[List[Any]] = None, top_k: int = 10, top_m: int = 3,
                filter_interacted: bool = True) -> Any:
        """An extension (the reference has none): [(item, [(reason_item, contribution), ...]), ...] -- SLIM.explain."""
        return self.model.explain(user, items, top_k=top_k, top_m=top_m, filter_interacted=filter_interacted)

    def explain_batch(self, users: List[Any], items: Optional[List[List[Any]]] = None, top_k: int = 10, top_m: int = 3,
                      filter_interacted: bool = True, as_arrays: bool = False) -> Any:
        """SLIM.explain_batch: recommend and explain in one device pass (`items=None`), or explain the given lists."""
        return self.model.explain_batch(users, items, top_k=top_k, top_m=top_m, filter_interacted=filter_interacted,
                                        as_arrays=as_arrays)

    def recommend_users(self, item: Any, top_n: int = 100, filter_interacted: bool = True,
                        candidate_users: Optional[List[Any]] = None, ret_scores: bool = False) -> Any:
        """An extension (the reference has none): the audience of an item, its top_n users by score -- SLIM.recommend_users."""
        return self.model.recommend_users(item, top_n=top_n, filter_interacted=filter_interacted, candidate_users=candidate_users,
                                          ret_scores=ret_scores)

    def recommend_users_batch(self, items: List[Any], top_n: int = 100, filter_interacted: bool = True,
                              candidate_users: Optional[List[Any]] = None, ret_scores: bool = False, as_arrays: bool = False) -> Any:
        """SLIM.recommend_users_batch: the audiences of many items in one device pass."""
        return self.model.recommend_users_batch(items, top_n=top_n, filter_interacted=filter_interacted,
                                                candidate_users=candidate_users, ret_scores=ret_scores, as_arrays=as_arrays)

    def rerank(self, user: Any, candidates: List[Any], top_k: Optional[int] = None, filter_interacted: bool = False,
               ret_scores: bool = False) -> Any:
        """An extension (the reference ranks one list for all users): the user's own candidates in rank order -- SLIM.rerank."""
        return self.model.rerank(user, candidates, top_k=top_k, filter_interacted=filter_interacted, ret_scores=ret_scores)

    def rerank_batch(self, users: List[Any], candidates: List[List[Any]], top_k: Optional[int] = None,
                     filter_interacted: bool = False, ret_scores: bool = False, as_arrays: bool = False) -> Any:
        """SLIM.rerank_batch: one candidate list per user, scored and ordered in one device pass."""
        return self.model.rerank_batch(users, candidates, top_k=top_k, filter_interacted=filter_interacted,
                                       ret_scores=ret_scores, as_arrays=as_arrays)

    def score_pairs(self, users: Any, items: Any, as_arrays: bool = False) -> Any:
        """SLIM.score_pairs: the model's score of every (users[p], items[p]) pair, and with `as_arrays` its support."""
        return self.model.score_pairs(users, items, as_arrays=as_arrays)

    def recommend_diverse(self, user: Any, top_k: int = 10, pool: int = 50, diversity: float = 0.3, filter_interacted: bool = True,
                          ret_scores: bool = False) -> Any:
        """An extension (the reference has none): the user's list re-ranked against W's similarities -- SLIM.recommend_diverse."""
        return self.model.recommend_diverse(user, top_k=top_k, pool=pool, diversity=diversity, filter_interacted=filter_interacted,
                                            ret_scores=ret_scores)

    def recommend_diverse_batch(self, users: List[Any], top_k: int = 10, pool: int = 50, diversity: float = 0.3,
                                filter_interacted: bool = True, ret_scores: bool = False, as_arrays: bool = False) -> Any:
        """SLIM.recommend_diverse_batch: score a pool per user and choose top_k of it greedily, in one device pass."""
        return self.model.recommend_diverse_batch(users, top_k=top_k, pool=pool, diversity=diversity,
                                                  filter_interacted=filter_interacted, ret_scores=ret_scores, as_arrays=as_arrays)

    def diversify_batch(self, items: List[List[Any]], scores: List[List[float]], top_k: int = 10, diversity: float = 0.3,
                        as_arrays: bool = False) -> Any:
        """SLIM.diversify_batch: the same selection for lists (and base scores) the caller brings."""
        return self.model.diversify_batch(items, scores, top_k=top_k, diversity=diversity, as_arrays=as_arrays)

    def recommend_blended(self, user: Any, other_items: List[Any], other_scores: List[float], top_k: int = 10, pool: Optional[int] = None,
                          weighting: Any = "contacts", contact_counts: Any = None, similarity_weight_factor: float = 2.0,
                          mnz: bool = False, filter_interacted: bool = True) -> List[Any]:
        """The user's SLIM list merged with a second scorer's list the way the reference's hybrid merges -- SLIM.recommend_blended."""
        return self.model.recommend_blended(user, other_items, other_scores, top_k=top_k, pool=pool, weighting=weighting,
                                            contact_counts=contact_counts, similarity_weight_factor=similarity_weight_factor, mnz=mnz,
                                            filter_interacted=filter_interacted)

    def recommend_blended_batch(self, users: List[Any], other_items: List[List[Any]], other_scores: List[List[float]], top_k: int = 10,
                                pool: Optional[int] = None, weighting: Any = "contacts", contact_counts: Any = None,
                                similarity_weight_factor: float = 2.0, mnz: bool = False, filter_interacted: bool = True,
                                as_arrays: bool = False) -> Any:
        """SLIM.recommend_blended_batch: score SLIM's lists and blend them with the brought ones, in one device pass."""
        return self.model.recommend_blended_batch(users, other_items, other_scores, top_k=top_k, pool=pool, weighting=weighting,
                                                  contact_counts=contact_counts, similarity_weight_factor=similarity_weight_factor,
                                                  mnz=mnz, filter_interacted=filter_interacted, as_arrays=as_arrays)

    def attach_factors(self, users: List[Any], user_vectors: Any, items: List[Any], item_vectors: Any) -> "Recommender":
        """Bring the vectors of a factor model trained elsewhere (SLIM.attach_factors): the second scorer of recommend_hybrid."""
        self.model.attach_factors(users, user_vectors, items, item_vectors)
        return self

    def attach_feature_factors(self, users: List[Any], user_tags: List[Any], user_table: Any, items: List[Any], item_tags: List[Any],
                               item_table: Any, user_bias: Any = None, item_bias: Any = None) -> "Recommender":
        """Bring the per-feature tables of a factor model trained with tags (SLIM.attach_feature_factors): the vectors are computed
        on the device from the identity and tag rows, and `user_tags` of recommend_factor / recommend_hybrid work."""
        self.model.attach_feature_factors(users, user_tags, user_table, items, item_tags, item_table, user_bias=user_bias,
                                          item_bias=item_bias)
        return self

    def fit_factors(self, dim: int = 32, iterations: int = 15, regularization: float = 0.01, alpha: float = 1.0,
                    seed: int = 0, *, solver: str = "cholesky", cg_steps: int = 3) -> "Recommender":
        """Train the second scorer of recommend_hybrid on the device by implicit ALS (SLIM.fit_factors); solver="cg" trains up
        to 256 components by `cg_steps` conjugate-gradient steps per row."""
        self.model.fit_factors(dim=dim, iterations=iterations, regularization=regularization, alpha=alpha, seed=seed,
                               solver=solver, cg_steps=cg_steps)
        return self

    def update_factors(self, users: List[Any], *, solver: Optional[str] = None, cg_steps: Optional[int] = None) -> "Recommender":
        """Solve the named users' vectors again after new interactions (SLIM.update_factors)."""
        self.model.update_factors(users, solver=solver, cg_steps=cg_steps)
        return self

    def detach_factors(self) -> "Recommender":
        self.model.detach_factors()
        return self

    def recommend_factor(self, user: Any, top_k: int = 10, filter_interacted: bool = True,
                         candidate_items: Optional[List[Any]] = None, user_tags: Optional[List[Any]] = None) -> List[Any]:
        """The attached factor model's own top-k for one user -- SLIM.recommend_factor."""
        kw = {} if user_tags is None else {"user_tags": user_tags}
        return self.model.recommend_factor(user, top_k=top_k, filter_interacted=filter_interacted, candidate_items=candidate_items, **kw)

    def recommend_factor_batch(self, users: List[Any], top_k: int = 10, filter_interacted: bool = True,
                               candidate_items: Optional[List[Any]] = None, as_arrays: bool = False,
                               users_tags: Optional[List[List[Any]]] = None) -> Any:
        """SLIM.recommend_factor_batch: dense vectors against dense vectors, top-k per user, one device pass."""
        kw = {} if users_tags is None else {"users_tags": users_tags}
        return self.model.recommend_factor_batch(users, top_k=top_k, filter_interacted=filter_interacted,
                                                 candidate_items=candidate_items, as_arrays=as_arrays, **kw)

    def recommend_hybrid(self, user: Any, top_k: int = 10, pool: Optional[int] = None, weighting: Any = "contacts",
                         contact_counts: Any = None, similarity_weight_factor: float = 2.0, mnz: bool = False,
                         filter_interacted: bool = True, user_tags: Optional[List[Any]] = None) -> List[Any]:
        """The reference's hybrid list for one user: the factor model's list blended with SLIM's -- SLIM.recommend_hybrid."""
        kw = {} if user_tags is None else {"user_tags": user_tags}
        return self.model.recommend_hybrid(user, top_k=top_k, pool=pool, weighting=weighting, contact_counts=contact_counts,
                                           similarity_weight_factor=similarity_weight_factor, mnz=mnz,
                                           filter_interacted=filter_interacted, **kw)

    def recommend_hybrid_batch(self, users: List[Any], top_k: int = 10, pool: Optional[int] = None, weighting: Any = "contacts",
                               contact_counts: Any = None, similarity_weight_factor: float = 2.0, mnz: bool = False,
                               filter_interacted: bool = True, as_arrays: bool = False,
                               users_tags: Optional[List[List[Any]]] = None) -> Any:
        """SLIM.recommend_hybrid_batch: factor top-k, SLIM's lists and the blend in one device pass."""
        kw = {} if users_tags is None else {"users_tags": users_tags}
        return self.model.recommend_hybrid_batch(users, top_k=top_k, pool=pool, weighting=weighting, contact_counts=contact_counts,
                                                 similarity_weight_factor=similarity_weight_factor, mnz=mnz,
                                                 filter_interacted=filter_interacted, as_arrays=as_arrays, **kw)

    def similar_items_factor(self, query_item: Any, top_k: int = 10, query_item_tags: Optional[List[Any]] = None,
                             first_component: Optional[int] = None) -> List[Any]:
        """The attached item vectors' own "more like this": (item, cosine) pairs -- SLIM.similar_items_factor."""
        kw = {} if query_item_tags is None else {"query_item_tags": query_item_tags}
        return self.model.similar_items_factor(query_item, top_k=top_k, first_component=first_component, **kw)

    def similar_items_factor_batch(self, query_items: List[Any], top_k: int = 10, query_items_tags: Optional[List[List[Any]]] = None,
                                   first_component: Optional[int] = None, as_arrays: bool = False) -> Any:
        """SLIM.similar_items_factor_batch: cosine top-k of item vectors against the catalogue, one device pass."""
        kw = {} if query_items_tags is None else {"query_items_tags": query_items_tags}
        return self.model.similar_items_factor_batch(query_items, top_k=top_k, first_component=first_component, as_arrays=as_arrays, **kw)

    def similar_items_hybrid(self, query_item: Any, top_k: int = 10, pool: Optional[int] = None,
                             query_item_tags: Optional[List[Any]] = None, first_component: Optional[int] = None) -> List[Any]:
        """The reference hybrid's similar_items for one item: (item, float) pairs -- SLIM.similar_items_hybrid."""
        kw = {} if query_item_tags is None else {"query_item_tags": query_item_tags}
        return self.model.similar_items_hybrid(query_item, top_k=top_k, pool=pool, first_component=first_component, **kw)

    def similar_items_hybrid_batch(self, query_items: List[Any], top_k: int = 10, pool: Optional[int] = None,
                                   query_items_tags: Optional[List[List[Any]]] = None, first_component: Optional[int] = None,
                                   as_arrays: bool = False) -> Any:
        """SLIM.similar_items_hybrid_batch: factor cosine top-k, W's column top-k and the float64 blend in one device pass."""
        kw = {} if query_items_tags is None else {"query_items_tags": query_items_tags}
        return self.model.similar_items_hybrid_batch(query_items, top_k=top_k, pool=pool, first_component=first_component,
                                                     as_arrays=as_arrays, **kw)

    def blend_batch(self, items_a: List[List[Any]], scores_a: List[List[float]], items_b: List[List[Any]], scores_b: List[List[float]],
                    top_k: int = 10, weight: float = 1.0, mnz: bool = False) -> Any:
        """SLIM.blend_batch: the same blend for two lists per row the caller brings, with a constant weight."""
        return self.model.blend_batch(items_a, scores_a, items_b, scores_b, top_k=top_k, weight=weight, mnz=mnz)

    def list_quality(self, items: List[Any]) -> Dict[str, Any]:
        """An extension (the reference has none): {n, intra_list_similarity, linked_pairs, novelty} of one list -- SLIM.list_quality."""
        return self.model.list_quality(items)

    def list_quality_batch(self, items: List[List[Any]], as_arrays: bool = False) -> Any:
        """SLIM.list_quality_batch: the same for many lists the caller brings, in one device pass."""
        return self.model.list_quality_batch(items, as_arrays=as_arrays)

    def recommend_quality(self, users: List[Any], top_k: int = 10, diversity: float = 0.0, pool: int = 50,
                          filter_interacted: bool = True, per_user: bool = False) -> Any:
        """SLIM.recommend_quality: intra-list similarity, novelty and catalogue exposure of the lists these users would be served."""
        return self.model.recommend_quality(users, top_k=top_k, diversity=diversity, pool=pool, filter_interacted=filter_interacted,
                                            per_user=per_user)

    def rank_items(self, user: Any, items: List[Any], filter_interacted: bool = True) -> Dict[str, Any]:
        """An extension (the reference has none): where `items` stand in the whole catalogue for `user` -- SLIM.rank_items."""
        return self.model.rank_items(user, items, filter_interacted=filter_interacted)

    def rank_items_batch(self, users: List[Any], items: List[List[Any]], filter_interacted: bool = True,
                         as_arrays: bool = False) -> Any:
        """SLIM.rank_items_batch: the same for many users, each with its own items, in passes over the resident X."""
        return self.model.rank_items_batch(users, items, filter_interacted=filter_interacted, as_arrays=as_arrays)

    def evaluate_catalogue(self, test_data: pd.DataFrame, ks: Sequence[int] = CATALOGUE_KS, filter_interacted: bool = True,
                           per_user: bool = False) -> Any:
        """An extension (the reference has none): accuracy over the WHOLE catalogue instead of the first recommend_size <= 64
        entries.  Every held-out (user, item) of test_data (columns user, item) gets its exact position among all the items
        `recommend(filter_interacted=...)` could list for the user (SLIM.rank_items_batch, csrc/catalogue_ranks.hip: counts on
        the device, no sort, no score matrix on the host), and utils.metrics.catalogue_rank_summary turns the positions into
        recall@k / hit_rate@k / ndcg@k for every k of `ks` in one pass, mrr, the exact auc and mean_percentile_rank, with the
        counts n_users, n_targets, tied_targets, never_listed, auc_users, unknown_items and skipped_users.  Per user the
        targets are its distinct held-out items the model has a column for; others are dropped and counted in unknown_items;
        users the model has no row for, or with no target left, are skipped and counted.  Ties are judged pessimistically (rank
        = above + tied).  `per_user=True` returns `(dict, frame)`: the per-user figures indexed by user in evaluation order."""
        hook = getattr(self.model, "_evaluate_catalogue", None)
        if hook is None:
            raise ValueError(f"evaluate_catalogue: {type(self.model).__name__} has no catalogue-rank hook")
        users, tg_ptr, above, tied, score, competing, unknown, skipped = hook(test_data["user"].to_numpy(), test_data["item"].to_numpy(),
                                                                              bool(filter_interacted))
        summary, cols = catalogue_rank_summary(tg_ptr, above, tied, score, competing, ks=ks, unknown_items=unknown,
                                               skipped_users=skipped)
        if per_user:
            return summary, pd.DataFrame(cols, index=pd.Index(users, name="user"))
        return summary

    def similar_items(self, query_items: List[Any], query_item_tags: Optional[List[str]] = None, top_k: int = 10,
                      ret_scores: bool = False):
        batch = getattr(self.model, "similar_items_batch", None)
        if batch is not None:        # one kernel launch for all queries instead of one per query
            return batch(query_items, query_item_tags, top_k, ret_scores)
        return [self.model.similar_items(item, query_item_tags, top_k, ret_scores) for item in query_items]

    def evaluate(self, test_data: pd.DataFrame, user_tags: Optional[Dict[Any, List[str]]] = None,
                 recommend_size: int = 10, batch_size=100, filter_interacted: bool = True,
                 on_device: bool = False, per_user: bool = False, diversity: float = 0.0, pool: int = 50,
                 list_quality: bool = False) -> Any:
        """Average ranking metrics over the users of test_data (columns user, item).

        `on_device=True` (extension) evaluates without leaving the GPU: the held-out items go up once, all users are scored
        in one pass, csrc/rank_metrics.hip turns (lists, ground truth) into the per-user figures and only those come back;
        the dict equals the host path's bit for bit.  `batch_size` has no effect there.  What that path does not serve --
        `user_tags`, a `recommend_size` outside 1..64 or beyond the fused top-k kernels, a model without the device hook, id
        columns that are neither integer nor object dtype, users that only the host path can place -- raises ValueError
        naming the reason: drop `on_device` then.
        `per_user=True` (extension, either path) returns `(dict, frame)`: the frame holds the nine figures per user, indexed
        by user in evaluation order (the order the means are summed in).
        `diversity > 0` (extension, `on_device=True` only) judges the lists of `recommend_diverse_batch(top_k=recommend_size,
        pool=pool, diversity=diversity)` instead, so the nine figures price the knob; `list_quality=True` (`on_device=True`
        only) adds the keys of `SLIM.recommend_quality` (utils.metrics.QUALITY_KEYS) for the same lists, computed in the same
        pass, and its four per-user columns to the frame.  With the defaults nothing changes."""
        if (diversity != 0.0 or list_quality) and not on_device:
            raise ValueError("evaluate: diversity and list_quality are served by the device path only: pass on_device=True")
        if on_device:
            return self._evaluate_on_device(test_data, user_tags, recommend_size, filter_interacted, per_user, diversity, pool,
                                            list_quality)
        truth = test_data.groupby("user")["item"].apply(list).to_dict()
        users = list(truth.keys())

        def pairs() -> Iterator[Tuple[List[Any], List[Any]]]:
            for s in range(0, len(users), batch_size):
                chunk = users[s:s + batch_size]
                tags = [user_tags.get(u, []) for u in chunk] if user_tags else None
                recs = self.recommend_batch(chunk, users_tags=tags, top_k=recommend_size,
                                            filter_interacted=filter_interacted)
                for u, rec in zip(chunk, recs):
                    yield rec, truth[u]
        if not per_user:
            return compute_scores(pairs(), recommend_size)
        rows = [_query_metrics(rec, tru, recommend_size) for rec, tru in pairs()]
        frame = pd.DataFrame(rows, index=pd.Index(users, name="user"), columns=list(RESULT_KEYS))
        return self._scores_and_frame(frame[list(METRIC_COLUMNS)].to_numpy(dtype=np.float64).reshape(len(users), 8),
                                      frame["tp"].to_numpy(dtype=np.int64), frame.index)

    @staticmethod
    def _scores_and_frame(metrics: np.ndarray, tp: np.ndarray, index: pd.Index) -> Tuple[Dict[str, float], pd.DataFrame]:
        frame = pd.DataFrame(metrics, index=index, columns=list(METRIC_COLUMNS))
        frame.insert(RESULT_KEYS.index("tp"), "tp", np.asarray(tp, dtype=np.int64))
        return scores_from_columns(metrics, tp), frame

    def _evaluate_on_device(self, test_data: pd.DataFrame, user_tags, recommend_size, filter_interacted: bool,
                            per_user: bool, diversity: float = 0.0, pool: int = 50, list_quality: bool = False) -> Any:
        if user_tags:
            raise ValueError("on_device evaluation does not take user_tags")
        if isinstance(recommend_size, bool) or not isinstance(recommend_size, (int, np.integer)) or not 1 <= recommend_size <= 64:
            raise ValueError(f"on_device evaluation serves an integer recommend_size in 1..64, got {recommend_size!r}")
        hook = getattr(self.model, "_evaluate_device", None)
        if hook is None:
            raise ValueError(f"on_device evaluation: {type(self.model).__name__} has no device evaluation hook")
        if diversity == 0.0 and not list_quality:
            users, metrics, tp, _ = hook(test_data["user"].to_numpy(), test_data["item"].to_numpy(), int(recommend_size),
                                         bool(filter_interacted))
            if per_user:
                return self._scores_and_frame(metrics, tp, pd.Index(users, name="user"))
            return scores_from_columns(metrics, tp)
        out = hook(test_data["user"].to_numpy(), test_data["item"].to_numpy(), int(recommend_size), bool(filter_interacted),
                   diversity=diversity, pool=pool, list_quality=bool(list_quality))
        users, metrics, tp = out[:3]
        scores, frame = self._scores_and_frame(metrics, tp, pd.Index(users, name="user"))
        scores = dict(scores)                       # (no user at all: compute_scores' empty defaultdict)
        if list_quality:
            n, sim_sum, linked, weight_sum, exposure = out[4]
            scores.update(quality_summary(n, sim_sum, linked, weight_sum, exposure))
            for name, col in quality_frame_columns(n, sim_sum, linked, weight_sum).items():
                frame[name] = col
        return (scores, frame) if per_user else scores

    @staticmethod
    def generate_batches(df: pd.DataFrame, batch_size: int = 1_000, as_generator: bool = False
                         ) -> Iterator[Iterable[Tuple[int, int, int, float]]]:
        """Mini-batches of (user, item, tstamp, rating) tuples in row order."""
        cols = [df[c].tolist() for c in df.columns[:4]]
        for s in range(0, len(df), batch_size):
            batch = list(zip(*(c[s:s + batch_size] for c in cols)))
            yield iter(batch) if as_generator else batch
