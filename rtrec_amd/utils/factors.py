"""Helpers for the factor scorer (SLIM.attach_factors, SlimEngine.set_factors): pure numpy."""
from __future__ import annotations

from typing import Tuple

import numpy as np


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
