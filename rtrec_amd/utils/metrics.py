"""Ranking metrics for Recommender.evaluate.

Definitions follow rtrec.utils.metrics (/root/reference/rtrec/utils/metrics.py:5-313): every
metric is a function of the 0/1 relevance vector of the first k = min(len(ranked), size)
recommendations and of |ground truth|; compute_scores averages them over queries.  Here the
relevance vector is formed once per query and all nine figures are derived from it.
"""
from __future__ import annotations

from collections import defaultdict
from math import log2
from typing import Any, Callable, Dict, Iterable, List, Sequence, Tuple

import numpy as np

METRIC_COLUMNS = ("precision", "recall", "f1", "ndcg", "hit_rate", "mrr", "map", "auc")     # rank_metrics_kernel's order
RESULT_KEYS = ("precision", "recall", "f1", "ndcg", "hit_rate", "mrr", "map", "tp", "auc")   # _query_metrics' order


def _relevance(ranked_list: Sequence[Any], ground_truth: Sequence[Any], size: int) -> List[int]:
    truth = set(ground_truth) if not isinstance(ground_truth, (set, frozenset)) else ground_truth
    return [1 if item in truth else 0 for item in ranked_list[:min(len(ranked_list), size)]]


def _query_metrics(ranked_list: Sequence[Any], ground_truth: Sequence[Any], size: int) -> Dict[str, float]:
    rel = _relevance(ranked_list, ground_truth, size)
    k, n_true, tp = len(rel), len(ground_truth), sum(rel)
    empty_truth = n_true == 0
    both_empty_score = 1.0 if not ranked_list else 0.0

    prec = both_empty_score if empty_truth else (tp / k if k else 0.0)
    rec = both_empty_score if empty_truth else tp / n_true
    if empty_truth and not ranked_list:
        f1 = 1.0
    else:
        f1 = 2 * prec * rec / (prec + rec) if (prec + rec) > 0 else 0.0

    dcg = sum(1.0 / log2(pos + 2) for pos, r in enumerate(rel) if r)
    idcg = sum(1.0 / log2(pos + 2) for pos in range(min(n_true, size)))
    first = next((pos for pos, r in enumerate(rel) if r), None)

    running, ap_sum, ordered_pairs = 0, 0.0, 0
    for pos, r in enumerate(rel):
        if r:
            running += 1
            ap_sum += running / (pos + 1)
        else:
            ordered_pairs += running          # every earlier hit outranks this miss
    if empty_truth:
        ap = auc = both_empty_score
    else:
        denom = min(n_true, size)
        ap = ap_sum / denom if denom else 0.0
        if not ranked_list or tp == 0:
            auc = 0.0
        elif tp == k:
            auc = 1.0
        else:
            auc = ordered_pairs / (tp * (k - tp))
    return {"precision": prec, "recall": rec, "f1": f1, "ndcg": dcg / idcg if idcg > 0 else 0.0,
            "hit_rate": 1.0 if tp else 0.0, "mrr": 0.0 if first is None else 1.0 / (first + 1),
            "map": ap, "tp": tp, "auc": auc}


def ndcg(ranked_list, ground_truth, recommend_size): return _query_metrics(ranked_list, ground_truth, recommend_size)["ndcg"]
def precision(ranked_list, ground_truth, recommend_size): return _query_metrics(ranked_list, ground_truth, recommend_size)["precision"]
def recall(ranked_list, ground_truth, recommend_size): return _query_metrics(ranked_list, ground_truth, recommend_size)["recall"]
def true_positives(ranked_list, ground_truth, recommend_size): return _query_metrics(ranked_list, ground_truth, recommend_size)["tp"]
def f1_score(ranked_list, ground_truth, recommend_size): return _query_metrics(ranked_list, ground_truth, recommend_size)["f1"]
def hit(ranked_list, ground_truth, recommend_size): return _query_metrics(ranked_list, ground_truth, recommend_size)["hit_rate"]
def reciprocal_rank(ranked_list, ground_truth, recommend_size): return _query_metrics(ranked_list, ground_truth, recommend_size)["mrr"]
def auc(ranked_list, ground_truth, recommend_size): return _query_metrics(ranked_list, ground_truth, recommend_size)["auc"]
def average_precision(ranked_list, ground_truth, recommend_size): return _query_metrics(ranked_list, ground_truth, recommend_size)["map"]


def _mean_over_queries(key: str, ranked_lists, ground_truths, size: int) -> float:
    vals = [_query_metrics(r, g, size)[key] for r, g in zip(ranked_lists, ground_truths)]
    return sum(vals) / len(vals) if vals else 0.0


def mrr(ranked_lists, ground_truths, recommend_size): return _mean_over_queries("mrr", ranked_lists, ground_truths, recommend_size)
def map_score(ranked_lists, ground_truths, recommend_size): return _mean_over_queries("map", ranked_lists, ground_truths, recommend_size)


def compute_scores(evaluation_pairs: Iterable[Tuple[List[Any], List[Any]]], recommend_size: int) -> Dict[str, float]:
    totals: Dict[str, float] = defaultdict(float)
    n = 0
    for ranked_list, ground_truth in evaluation_pairs:
        n += 1
        for name, value in _query_metrics(ranked_list, ground_truth, recommend_size).items():
            totals[name] += value
    if n == 0:
        return defaultdict(float)
    return {name: (int(total) if name == "tp" else total / n) for name, total in totals.items()}


# ---------------------------------------------------------------------------------------------------------------------
# Array forms for Recommender.evaluate: the ground truth as CSR (what rank_metrics_kernel reads), the discount tables the
# device cannot compute itself (no libm there), and compute_scores' means over per-user columns.

def discount_tables(size: int) -> Tuple[np.ndarray, np.ndarray]:
    """(discount[size], ideal[size + 1]): discount[i] = 1 / log2(i + 2) with Python's math.log2 -- the addends of dcg --
    and ideal[m] = the idcg of min(len(ground_truth), size) == m, summed left to right from 0 like `sum(...)` does."""
    discount = [1.0 / log2(pos + 2) for pos in range(size)]
    ideal = [0.0]
    for d in discount:
        ideal.append(ideal[-1] + d)
    return np.asarray(discount, dtype=np.float64), np.asarray(ideal, dtype=np.float64)


def sequential_sum(values: np.ndarray) -> float:
    """((0 + v[0]) + v[1]) + ... in float64: compute_scores' `totals[name] += value` loop.  np.cumsum accumulates in
    order; np.sum adds pairwise and differs in the last bits."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    return float(np.cumsum(values)[-1]) if len(values) else 0.0


def _missing(column: np.ndarray) -> np.ndarray:
    """The keys pandas' groupby drops: NaN, and None in an object column."""
    if column.dtype.kind == "f":
        return np.isnan(column)
    if column.dtype.kind == "O":
        return np.not_equal(column, column).astype(bool) | np.equal(column, None).astype(bool)
    return np.zeros(len(column), dtype=bool)


def _distinct(values: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """np.unique(values, return_inverse=True).  Small non-negative integers -- pass-through ids -- are counted instead of
    sorted (a bincount and a gather instead of an argsort over every row of the frame)."""
    if values.dtype.kind in "iu" and len(values):
        lo, hi = int(values.min()), int(values.max())
        if lo >= 0 and hi <= 4 * len(values) + 65536:
            seen = np.bincount(values, minlength=hi + 1) > 0
            return np.flatnonzero(seen).astype(values.dtype), (np.cumsum(seen) - 1)[values]
    return np.unique(values, return_inverse=True)


def ground_truth_csr(users: np.ndarray, items: np.ndarray, user_index: Callable[[np.ndarray], np.ndarray],
                     item_index: Callable[[np.ndarray], np.ndarray]):
    """The dict `frame.groupby("user")["item"].apply(list).to_dict()` of Recommender.evaluate as arrays.

    `users` / `items` are the two id columns; `user_index(distinct users)` / `item_index(distinct items)` return the
    internal int64 id of every distinct value, -1 for one the model does not know.  Returns
        eval_users   the distinct users in evaluation order (groupby sorts its keys and drops missing ones)
        user_rows    their internal ids (-1: unknown user)
        truth_ptr    int64[n + 1], truth_items int32: per user the KNOWN items of its list, sorted and unique
        truth_len    int32[n]: len() of the user's list -- duplicated rows and unknown items included, which is what the
                     reference divides by while it tests membership against the list's distinct values
    One sort per column and one over the (user, item) pairs; no Python object per row."""
    users, items = np.asarray(users), np.asarray(items)
    if users.shape != items.shape or users.ndim != 1:
        raise ValueError("users and items must be two columns of one length")
    drop = _missing(users)
    if drop.any():
        users, items = users[~drop], items[~drop]
    eval_users, u_pos = _distinct(users)
    n = len(eval_users)
    user_rows = np.asarray(user_index(eval_users), dtype=np.int64) if n else np.empty(0, np.int64)
    truth_len = np.bincount(u_pos, minlength=n).astype(np.int32)
    ok = ~_missing(items)                       # a missing item is in the list (it counts) but equals no recommendation
    distinct, i_pos = _distinct(items if ok.all() else items[ok])
    ids = np.asarray(item_index(distinct), dtype=np.int64) if len(distinct) else np.empty(0, np.int64)
    item_ids, rows = ids[i_pos], (u_pos if ok.all() else u_pos[ok])
    known = item_ids >= 0
    if known.any():
        if not known.all():
            rows, item_ids = rows[known], item_ids[known]
        bound = int(item_ids.max()) + 1
        rows, truth_items = np.divmod(np.unique(rows.astype(np.int64, copy=False) * bound + item_ids), bound)
        truth_items = truth_items.astype(np.int32)
    else:
        rows, truth_items = np.empty(0, np.int64), np.empty(0, np.int32)
    truth_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=truth_ptr[1:])
    return eval_users, user_rows, truth_ptr, truth_items, truth_len


def scores_from_columns(metrics: np.ndarray, tp: np.ndarray) -> Dict[str, float]:
    """compute_scores over per-user columns (metrics[n, 8] in METRIC_COLUMNS order, tp[n]): sequential float64 sums in row
    order divided by n, tp an integer sum; the same dict, key order included."""
    n = len(tp)
    if n == 0:
        return defaultdict(float)
    col = {name: sequential_sum(metrics[:, j]) / n for j, name in enumerate(METRIC_COLUMNS)}
    col["tp"] = int(np.asarray(tp, dtype=np.int64).sum())
    return {name: col[name] for name in RESULT_KEYS}


# ---------------------------------------------------------------------------------------------------------------------
# List quality (csrc/list_quality.hip): what a served list looks like apart from its accuracy.  The kernel returns four raw
# figures per list and one exposure count per item; everything below is pure host arithmetic over them.

QUALITY_COLUMNS = ("n", "intra_list_similarity", "linked_pairs", "novelty")            # the per-list figures, as the frames carry them
QUALITY_KEYS = ("n_lists", "n_lists_nonempty", "n_lists_pairs", "mean_length", "intra_list_similarity", "linked_share", "novelty",
                "distinct_items", "coverage", "gini")


def novelty_weights(pop: np.ndarray, n_users: int, n_items: int) -> np.ndarray:
    """float32[n_items]: the self-information log2(n_users) - log2(max(pop_i, 1)) of every item, computed in float64 and rounded
    once; `pop` (the stored entries per column of X) is cut or zero-padded to n_items, so an item X has never seen weighs like
    one seen once.  (No user at all counts as one: the table is then all zeros rather than -inf.)"""
    pop = np.asarray(pop, dtype=np.int64)[:n_items]
    if len(pop) < n_items:
        pop = np.concatenate([pop, np.zeros(n_items - len(pop), dtype=np.int64)])
    return (np.log2(np.float64(max(int(n_users), 1))) - np.log2(np.maximum(pop, 1).astype(np.float64))).astype(np.float32)


def list_quality_figures(n: np.ndarray, sim_sum: np.ndarray, linked: np.ndarray, weight_sum: np.ndarray
                         ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per list (float64 arrays): intra_list_similarity = sim_sum / (m (m - 1) / 2) and linked_share = linked / that number of
    pairs for m >= 2, novelty = weight_sum / m for m >= 1; NaN where a figure is not defined."""
    m = np.asarray(n, dtype=np.int64)
    pairs = (m * (m - 1) // 2).astype(np.float64)
    ils = np.full(len(m), np.nan)
    share = np.full(len(m), np.nan)
    nov = np.full(len(m), np.nan)
    two, one = m >= 2, m >= 1
    with np.errstate(invalid="ignore", over="ignore"):
        ils[two] = np.asarray(sim_sum, dtype=np.float32)[two].astype(np.float64) / pairs[two]
        share[two] = np.asarray(linked, dtype=np.int64)[two].astype(np.float64) / pairs[two]
        nov[one] = np.asarray(weight_sum, dtype=np.float32)[one].astype(np.float64) / m[one].astype(np.float64)
    return ils, share, nov


def fsum_mean(values: np.ndarray) -> float:
    """math.fsum(values) / len(values): the exactly rounded sum, so the mean does not depend on the order; NaN for no value."""
    from math import fsum
    values = np.asarray(values, dtype=np.float64)
    if len(values) == 0:
        return float("nan")
    with np.errstate(invalid="ignore"):
        try:
            return fsum(values.tolist()) / len(values)
        except (OverflowError, ValueError):     # (inf - inf, or a sum beyond the doubles: fsum raises where + would give nan / inf)
            return float(np.sum(values) / len(values))


def gini(exposure: np.ndarray) -> float:
    """The Gini coefficient of an exposure count per item, never-shown items counting as 0: with e ascending and i = 1..n,
    sum_i (2 i - n - 1) e_i / (n sum_i e_i), numerator and denominator as exact integers and one correctly rounded division.
    0 for a uniform exposure, (n - 1) / n for a single item; NaN when nothing was shown."""
    e = np.sort(np.asarray(exposure).astype(np.int64).ravel())
    n = len(e)
    total = int(e.sum(dtype=object)) if n else 0
    if total <= 0:
        return float("nan")
    coef = 2 * np.arange(1, n + 1, dtype=np.int64) - n - 1
    if n * total < 2 ** 62:
        num = int(np.dot(coef, e))
    else:
        num = int(np.dot(coef.astype(object), e.astype(object)))
    return num / (n * total)


def quality_summary(n: np.ndarray, sim_sum: np.ndarray, linked: np.ndarray, weight_sum: np.ndarray, exposure: np.ndarray
                    ) -> Dict[str, Any]:
    """The figures of a batch of lists, in QUALITY_KEYS order: n_lists (all of them, mean_length's count), n_lists_nonempty
    (m >= 1: novelty's count), n_lists_pairs (m >= 2: the count behind intra_list_similarity and linked_share); the fsum means
    of the per-list figures over the lists where each is defined (NaN over none); and the catalogue side of `exposure`
    [n_items]: distinct_items shown at all, coverage = distinct_items / n_items (NaN for an empty catalogue), gini."""
    m = np.asarray(n, dtype=np.int64)
    ils, share, nov = list_quality_figures(m, sim_sum, linked, weight_sum)
    exposure = np.asarray(exposure)
    distinct = int(np.count_nonzero(exposure > 0))
    out = {"n_lists": int(len(m)), "n_lists_nonempty": int((m >= 1).sum()), "n_lists_pairs": int((m >= 2).sum()),
           "mean_length": fsum_mean(m), "intra_list_similarity": fsum_mean(ils[m >= 2]), "linked_share": fsum_mean(share[m >= 2]),
           "novelty": fsum_mean(nov[m >= 1]), "distinct_items": distinct,
           "coverage": distinct / len(exposure) if len(exposure) else float("nan"), "gini": gini(exposure)}
    return {key: out[key] for key in QUALITY_KEYS}


def quality_frame_columns(n: np.ndarray, sim_sum: np.ndarray, linked: np.ndarray, weight_sum: np.ndarray) -> Dict[str, np.ndarray]:
    """The per-list columns in QUALITY_COLUMNS order: n and linked_pairs as int64, the two ratios as float64."""
    ils, _, nov = list_quality_figures(n, sim_sum, linked, weight_sum)
    return {"n": np.asarray(n, dtype=np.int64), "intra_list_similarity": ils, "linked_pairs": np.asarray(linked, dtype=np.int64),
            "novelty": nov}


# ---------------------------------------------------------------------------------------------------------------------
# Catalogue ranks (csrc/catalogue_ranks.hip): where the held-out items stand in the WHOLE catalogue.  The kernel returns, per
# target, the competing columns above it and tied with it and its score, and per user the competing columns; everything below
# is pure host arithmetic over them, in float64.

CATALOGUE_KS = (1, 5, 10, 20, 50, 100)


def catalogue_rank_summary(tg_ptr: np.ndarray, above: np.ndarray, tied: np.ndarray, score: np.ndarray, competing: np.ndarray,
                           ks: Sequence[int] = CATALOGUE_KS, unknown_items: int = 0, skipped_users: int = 0
                           ) -> Tuple[Dict[str, Any], Dict[str, np.ndarray]]:
    """(summary, per-user columns) of the ranks of user u's targets tg_ptr[u] .. tg_ptr[u + 1] (distinct items): `above` / `tied`
    / `score` per target and `competing` per user as rtrec_slim_catalogue_ranks defines them (include/rtrec_amd_ext.h).

    A target with above == -1 can never be listed: it is a miss everywhere and counts in `never_listed`.  The integer rank
    of a listed target is the pessimistic above + tied, 0-based.  Per user, with P = its targets and k in `ks`:
        recall@k, hit_rate@k   the targets with rank < k, over P; whether there is one
        ndcg@k                 the sum of 1 / log2(rank + 2) over them in rank order, over the same sum for ranks
                               0 .. min(P, k) - 1 (utils.metrics.discount_tables)
        mrr                    1 / (best rank + 1) over the whole catalogue, 0 without a listed target
        auc                    mid-rank Mann-Whitney of the targets against the N = competing - listed targets negatives: a
                               listed target has neg_above = above - (the listed targets scoring higher) negatives above it and
                               neg_tied = tied - (the other listed targets scoring the same) tied with it, by the float64
                               scores; it contributes N - neg_above - neg_tied / 2, a never-listed one 0; the sum over P * N.
                               A user with N == 0 has no auc (NaN in the column) and is left out of the mean
        mean_percentile_rank   per target (neg_above + neg_tied / 2) / N, 1.0 for a never-listed one, 0.0 for a listed one
                               with N == 0: the share of the negatives that stand above it
    The summary holds the math.fsum means over the users in row order (auc over its `auc_users`; mean_percentile_rank over all
    `n_targets` targets), NaN over nothing, and the counts n_users, n_targets, tied_targets (listed, tied > 0), never_listed,
    auc_users, unknown_items and skipped_users -- the last two are the caller's, plus the rows that bring no target here."""
    tg_ptr = np.asarray(tg_ptr, dtype=np.int64)
    above, tied = np.asarray(above, dtype=np.int64), np.asarray(tied, dtype=np.int64)
    score, competing = np.asarray(score, dtype=np.float64), np.asarray(competing, dtype=np.int64)
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError(f"catalogue_rank_summary: every k must be at least 1, got {ks}")
    n_rows = len(tg_ptr) - 1
    P_all = np.diff(tg_ptr)
    keep = P_all > 0
    skipped_users = int(skipped_users) + int((~keep).sum())
    n, n_tg = int(keep.sum()), int(P_all.sum())
    u = np.repeat(np.cumsum(keep) - 1, P_all)                      # the kept user of every target
    P, comp = P_all[keep], competing[keep]
    above, tied, score = above[tg_ptr[0]:tg_ptr[-1]], tied[tg_ptr[0]:tg_ptr[-1]], score[tg_ptr[0]:tg_ptr[-1]]
    listed = above >= 0
    rank = np.where(listed, above + tied, np.iinfo(np.int64).max)
    n_listed = np.bincount(u[listed], minlength=n)
    N = comp - n_listed
    # the listed targets scoring higher than / the same as each listed target, inside its user: one sort by (user, score desc)
    pos_above, pos_tied = np.zeros(n_tg, np.int64), np.zeros(n_tg, np.int64)
    li = np.flatnonzero(listed)
    if len(li):
        order = li[np.lexsort((-score[li], u[li]))]
        su, ss = u[order], score[order]
        new_user = np.r_[True, su[1:] != su[:-1]]
        new_run = new_user | np.r_[True, ss[1:] != ss[:-1]]
        idx = np.arange(len(order))
        run_start = np.maximum.accumulate(np.where(new_run, idx, 0))
        user_start = np.maximum.accumulate(np.where(new_user, idx, 0))
        run_len = np.bincount(np.cumsum(new_run) - 1)[np.cumsum(new_run) - 1]
        pos_above[order], pos_tied[order] = run_start - user_start, run_len - 1
    neg_above, neg_tied = above - pos_above, tied - pos_tied
    Nt = N[u].astype(np.float64)
    mid = neg_above + 0.5 * neg_tied
    with np.errstate(invalid="ignore", divide="ignore"):
        pct = np.where(listed, np.where(Nt > 0, mid / Nt, 0.0), 1.0)
        wins = np.where(listed, Nt - mid, 0.0)
        auc_user = np.bincount(u, weights=wins, minlength=n) / (P * N.astype(np.float64))
    auc_user = np.where(N > 0, auc_user, np.nan)
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, u, rank)
    has = n_listed > 0
    cols: Dict[str, np.ndarray] = {"n_targets": P, "never_listed": P - n_listed, "competing": comp,
                                   "best_rank": np.where(has, best, -1),
                                   "mrr": np.where(has, 1.0 / (np.where(has, best, 0) + 1.0), 0.0), "auc": auc_user,
                                   "mean_percentile_rank": np.bincount(u, weights=pct, minlength=n) / np.maximum(P, 1)}
    by_rank = np.lexsort((rank, u))                                 # dcg adds its terms in rank order, like _query_metrics
    for k in ks:
        _, ideal = discount_tables(k)
        hit = rank < k
        tp = np.bincount(u[hit], minlength=n)
        sel = by_rank[hit[by_rank]]
        dcg = np.bincount(u[sel], weights=1.0 / np.log2(rank[sel] + 2.0), minlength=n)
        cols[f"recall@{k}"] = tp / np.maximum(P, 1)
        cols[f"hit_rate@{k}"] = (tp > 0).astype(np.float64)
        cols[f"ndcg@{k}"] = dcg / ideal[np.minimum(P, k)] if n else dcg
    out: Dict[str, Any] = {}
    for k in ks:
        for name in (f"recall@{k}", f"hit_rate@{k}", f"ndcg@{k}"):
            out[name] = fsum_mean(cols[name])
    out["mrr"] = fsum_mean(cols["mrr"])
    out["auc"] = fsum_mean(auc_user[N > 0])
    out["mean_percentile_rank"] = fsum_mean(pct)
    out.update({"n_users": n, "n_targets": n_tg, "tied_targets": int((listed & (tied > 0)).sum()),
                "never_listed": int((~listed).sum()), "auc_users": int((N > 0).sum()), "unknown_items": int(unknown_items),
                "skipped_users": skipped_users})
    return out, cols
