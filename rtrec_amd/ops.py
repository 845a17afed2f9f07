"""PyTorch-ROCm custom ops over the C-ABI (`torch.ops.rtrec_amd.*`), registered from C++.

One op per entry point of include/rtrec_amd.h, in out-variant style: every buffer is a ROCm tensor owned by the caller,
outputs and scratch are marked mutable in the schema, scalars are plain ints / floats / bools, and the work is enqueued on
the current stream of the tensors' device.  The ops only marshal pointers -- all computation is in librtrec_amd.so -- so
they compose with torch streams, the caching allocator and torch.distributed without copies.  rtrec_amd.engine.HipBackend
is written on top of them; they are also the interface for callers that already hold device tensors.

    torch.ops.rtrec_amd.column_sqnorms      norm_cols_X of the coordinate descent
    torch.ops.rtrec_amd.fit_workspace_init  scratch invariants of the fit kernel
    torch.ops.rtrec_amd.gram_matrix         Gram matrix of the popular items (Gram tracking)
    torch.ops.rtrec_amd.fit_columns         X^T y feature selection + elastic-net CD per item column
    torch.ops.rtrec_amd.score_topk          user rows x W shard, interacted filter, top-k
    torch.ops.rtrec_amd.score_rows          score vectors (predict*)
    torch.ops.rtrec_amd.merge_topk          per-tile / per-GPU top-k lists -> top-k
    torch.ops.rtrec_amd.similar_topk        similar_items
    torch.ops.rtrec_amd.store_decay_device  time decay of a resident store      .store_fold_device   bulk ingest: fold per (user, item)
    torch.ops.rtrec_amd.fit_sgd_epochs      optim="sgd" epochs                  .first_touch_aux     cross-shard tie key
    torch.ops.rtrec_amd.dense_fill          DENSE lists completed in place      .refine_topk_f64     float64 refine of a fast pass
    torch.ops.rtrec_amd.score_candidates    request-sized CANDIDATES calls      .seg_plan / .seg_fill  segment layout of a general W
    torch.ops.rtrec_amd.ordered_sums        left-to-right float32 sums (the fit kernels' fold, for tests and tools)
    torch.ops.rtrec_amd.rank_metrics        the nine ranking figures of Recommender.evaluate per user, from lists on the device
    torch.ops.rtrec_amd.explain_topk        per (user, item) of a top-k list: the top-m terms x_uj * w_ji of the score, and their number
    torch.ops.rtrec_amd.audience_topk       per query item: the top-n users by score (the scoring product read by W's column), and its reach
    torch.ops.rtrec_amd.score_pairs         per (user, item) of per-user candidate lists: the score and its support, and each list's order
    torch.ops.rtrec_amd.diversify_lists     (extension surface, include/rtrec_amd_ext.h) per list: the greedy MMR order over W's similarities
    torch.ops.rtrec_amd.list_quality        (extension surface) per list: intra-list similarity sum, linked pairs, weight sum; the catalogue exposure
    torch.ops.rtrec_amd.catalogue_ranks     (extension surface) per held-out (row, item): the columns of the dense score row above it and tied with it
    torch.ops.rtrec_amd.blend_lists         (extension surface) per row: the union of two lists, each min-max normalised, the second weighted per item, re-ranked
    torch.ops.rtrec_amd.factor_topk         (extension surface) per row: dense user vector x dense item vectors (f32 MFMA = the fmaf chain), filtered top-k, fused
    torch.ops.rtrec_amd.feature_repr        (extension surface) per job: sparse feature row x per-feature table (ordered, unfused float32 chain), written where factor_topk reads
    torch.ops.rtrec_amd.factor_norms        (extension surface) per vector: the Euclidean norm as the ordered fmaf chain of its squares, correctly rounded root
    torch.ops.rtrec_amd.factor_similar_topk (extension surface) per query item: cosine top-k against all item vectors (f32 MFMA, one division per score), the query excluded
    torch.ops.rtrec_amd.similar_blend       (extension surface) per row: two lists cut, the query taken out, min-max normalised, summed per id in float64, re-ranked
    torch.ops.rtrec_amd.factor_gram         (extension surface) V^T V + reg I of one side's vectors in chunks of 1024 rows (f32 MFMA = the fmaf chain), the partials added in order
    torch.ops.rtrec_amd.factor_als_solve    (extension surface) per row of R: G + sum w y y^T on the f32 MFMA, a pinned Cholesky solve, written in place; one status per job
    torch.ops.rtrec_amd.factor_gram_wide    (extension surface) factor_gram for vectors of up to 256 components: one MFMA chain per (chunk, lower 32 x 32 tile)
    torch.ops.rtrec_amd.factor_als_cg       (extension surface) per row of R: pinned conjugate-gradient steps on the same system, never formed; dim up to 256, warm start

The registration lives in csrc/torch_ops.cpp (TORCH_LIBRARY / TORCH_LIBRARY_IMPL: librtrec_amd_ops.so, built by
rtrec_amd/build.py with the host compiler); importing this module loads it and binds it to the C-ABI library
(`rtrec_ops_bind`: the build named by RTREC_AMD_LIB, or the in-tree one).  Round 2 registered the same schemas as Python
`torch.library.custom_op` bodies that called ctypes: a call now goes dispatcher -> C++ -> C-ABI without re-entering Python.
There is no fallback: without the ops library the import fails.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native
from . import build as _build

OPS = ["column_sqnorms", "fit_workspace_init", "gram_matrix", "fit_columns", "score_topk", "score_rows", "merge_topk",
       "similar_topk", "store_decay_device", "store_fold_device", "fit_sgd_epochs", "first_touch_aux", "dense_fill",
       "refine_topk_f64", "score_candidates", "seg_plan", "seg_fill", "ordered_sums", "rank_metrics", "explain_topk", "audience_topk",
       "score_pairs"]

# C-ABI export each op launches (tests: every kernel-launching export of include/rtrec_amd.h is behind an op)
EXPORT_OF = {"column_sqnorms": "rtrec_slim_column_sqnorms", "fit_workspace_init": "rtrec_slim_fit_workspace_init",
             "gram_matrix": "rtrec_slim_gram_matrix", "fit_columns": "rtrec_slim_fit_columns_opt",
             "score_topk": "rtrec_slim_score_topk_opt", "score_rows": "rtrec_slim_score_rows",
             "merge_topk": "rtrec_slim_merge_topk_strided", "similar_topk": "rtrec_slim_similar_topk",
             "store_decay_device": "rtrec_store_decay_device", "store_fold_device": "rtrec_store_fold_device",
             "fit_sgd_epochs": "rtrec_slim_fit_sgd_epochs", "first_touch_aux": "rtrec_slim_first_touch_aux",
             "dense_fill": "rtrec_slim_dense_fill", "refine_topk_f64": "rtrec_slim_refine_topk_f64",
             "score_candidates": "rtrec_slim_score_candidates", "seg_plan": "rtrec_slim_seg_plan", "seg_fill": "rtrec_slim_seg_fill",
             "ordered_sums": "rtrec_slim_ordered_sums", "rank_metrics": "rtrec_rank_metrics",
             "explain_topk": "rtrec_slim_explain_topk", "audience_topk": "rtrec_slim_audience_topk",
             "score_pairs": "rtrec_slim_score_pairs"}

# The extension surface (include/rtrec_amd_ext.h, _native.EXT_EXPORTS): the same rules -- one op per kernel-launching export
EXT_OPS = ["diversify_lists", "list_quality", "catalogue_ranks", "blend_lists", "factor_topk", "feature_repr",
           "factor_norms", "factor_similar_topk", "similar_blend", "factor_gram", "factor_als_solve", "factor_gram_wide", "factor_als_cg"]
EXT_EXPORT_OF = {"diversify_lists": "rtrec_slim_diversify_lists", "list_quality": "rtrec_slim_list_quality",
                 "catalogue_ranks": "rtrec_slim_catalogue_ranks", "blend_lists": "rtrec_slim_blend_lists",
                 "factor_topk": "rtrec_factor_topk", "feature_repr": "rtrec_feature_repr",
                 "factor_norms": "rtrec_factor_norms", "factor_similar_topk": "rtrec_factor_similar_topk",
                 "similar_blend": "rtrec_similar_blend", "factor_gram": "rtrec_factor_gram",
                 "factor_als_solve": "rtrec_factor_als_solve", "factor_gram_wide": "rtrec_factor_gram_wide",
                 "factor_als_cg": "rtrec_factor_als_cg"}


def _load() -> None:
    path = _build.OPS_PATH
    if not os.path.exists(path):
        raise _native.NativeLibraryError(
            f"{path} is missing: build it with `python -m rtrec_amd.build` (host compiler + torch headers). "
            "rtrec_amd has no Python fallback for its custom ops.")
    _native.load()                       # torch's HIP runtime first, then the C-ABI library
    torch.ops.load_library(path)
    lib = C.CDLL(path)
    lib.rtrec_ops_bind.restype = C.c_int
    lib.rtrec_ops_bind.argtypes = [C.c_char_p]
    rc = lib.rtrec_ops_bind(_native.lib_path().encode())
    if rc != 0:
        raise _native.NativeLibraryError(f"rtrec_ops_bind({_native.lib_path()}) failed ({rc}): the C-ABI library does not load "
                                         "or misses an entry point")


_load()
