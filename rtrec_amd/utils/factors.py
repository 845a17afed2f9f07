"""Helpers for the factor scorer (SLIM.attach_factors, SlimEngine.set_factors): pure numpy."""
from __future__ import annotations

from typing import Any, Iterable, List, Mapping, Sequence, Tuple

import numpy as np
from scipy.sparse import csr_matrix


def feature_rows(identity_cols: Sequence[int], tags: Sequence[Iterable[Any]], tag_cols: Mapping[Any, int], n_cols: int) -> csr_matrix:
    """The sparse feature rows the reference's hybrid model multiplies into LightFM's per-feature tables, one per entity
    (rtrec/models/hybrid.py: hstack((identity, FeatureStore.build_*_features_matrix(ids, tags)))[ids], and _cold_user_features
    for entities without an identity): a float32 CSR [len(identity_cols), n_cols].  Row r stores, in this order, the identity
    column `identity_cols[r]` with value 1 (a negative value: the entity has no identity row) and then the columns
    `tag_cols[t]` of its tags `tags[r]` in ascending column order, each with its multiplicity as the value (the reference's
    COO -> CSR conversion sums a tag named twice); a tag `tag_cols` does not know is skipped.  The order is part of the
    result: the representation kernel adds the entries as they are stored (csrc/feature_repr.hip)."""
    if len(identity_cols) != len(tags):
        raise ValueError(f"one tag list is needed per entity, got {len(identity_cols)} entities and {len(tags)} tag lists")
    indptr = np.zeros(len(tags) + 1, dtype=np.int64)
    cols: List[int] = []
    vals: List[float] = []
    for r, (ident, ts) in enumerate(zip(identity_cols, tags)):
        ident = int(ident)
        if ident >= n_cols:
            raise ValueError(f"identity column {ident} lies beyond the table's {n_cols} rows")
        if ident >= 0:
            cols.append(ident)
            vals.append(1.0)
        seen: dict = {}
        for t in ts:
            c = tag_cols.get(t)
            if c is not None:
                seen[c] = seen.get(c, 0) + 1
        for c in sorted(seen):
            cols.append(int(c))
            vals.append(float(seen[c]))
        indptr[r + 1] = len(cols)
    return csr_matrix((np.asarray(vals, dtype=np.float32), np.asarray(cols, dtype=np.int32), indptr.astype(np.int32)),
                      shape=(len(tags), int(n_cols)))


def stack_bias(user_bias, user_emb, item_bias, item_emb) -> Tuple[np.ndarray, np.ndarray]:
    """The two float32 matrices whose row dot products are b_u + b_i + e_u . e_i, in the layout the reference's hybrid model
    hands to its top-k call (rtrec/models/hybrid.py): user rows [b_u, 1, e_u...], item rows [1, b_i, e_i...].  `user_bias` [U],
    `user_emb` [U, d], `item_bias` [I], `item_emb` [I, d]; returns ([U, d + 2], [I, d + 2])."""
    user_bias = np.asarray(user_bias, dtype=np.float32).reshape(-1)
    item_bias = np.asarray(item_bias, dtype=np.float32).reshape(-1)
    user_emb = np.asarray(user_emb, dtype=np.float32)
    item_emb = np.asarray(item_emb, dtype=np.float32)
    if user_emb.ndim != 2 or item_emb.ndim != 2 or user_emb.shape[1] != item_emb.shape[1]:
        raise ValueError(f"user_emb and item_emb must be two matrices of one width, got {user_emb.shape} and {item_emb.shape}")
    if user_bias.shape[0] != user_emb.shape[0] or item_bias.shape[0] != item_emb.shape[0]:
        raise ValueError("one bias is needed per embedding row")
    users = np.hstack([user_bias[:, None], np.ones((len(user_bias), 1), dtype=np.float32), user_emb])
    items = np.hstack([np.ones((len(item_bias), 1), dtype=np.float32), item_bias[:, None], item_emb])
    return np.ascontiguousarray(users, dtype=np.float32), np.ascontiguousarray(items, dtype=np.float32)
