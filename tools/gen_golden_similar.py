#!/usr/bin/env python3
"""Writes tests/golden/similar_blend.json: what the reference's HybridSlimFM._similar_items answers after its top-k call.

Runs only where the reference is installed beside this repository (tools/ref_import.py); no test imports this file.  The REAL
method is called on an instance made WITHOUT its constructor (the constructor builds the LightFM half, which is not installed
and not needed).  The instance carries
  * `slim_model`: a stand-in whose similar_items(query, top_k, ret_ndarrays=True) answers from the case's list B -- for the
    fixture cases the column of the tests/golden W (rtrec_slim_similar_topk's rule: the larger value first, the lower row among
    equal ones);
  * `model.get_item_representations` and `_create_item_features`: stand-ins that return the case's seeded vectors;
  * `implicit.topk`, replaced in the reference module by a stand-in that returns the host model's (ids, s1) for the items, the
    query and the item_norms the method hands it (the cosine host model of tests/test_similar_host.py) -- or the case's list A.
Everything after the top-k is then the reference's own code under this machine's numpy: the cut at -FLT_MAX, / calc_norm(query),
the id mask, minmax_normalize on both lists, comb_sum and sorted(..., reverse=True)[:top_k].

Cases, in this order:
  * the 400 items of the tests/golden W (no column of it is empty, so the reference never raises) at top_k = 10, with seeded
    item vectors correlated with W: [bias, a rank-11 SVD of W + W^T] plus 0.02 normal noise, use_bias = True (the method's
    np.hstack);
  * 60 small seeded cases over 24 items: lengths 1..12, ids drawn WITH replacement (repeated ids in either list), every fifth
    list flat, scores scaled by 1e-9 and by 50 in turn, some A lists ending in implicit's -FLT_MAX marker, the query sometimes
    inside A; case 0 is the crafted one in which float32 addition would change the ORDER (tests/test_similar_host.order_case).

Per case the file holds both input lists (A with s1 scores, as the top-k returned them), the query, the query norm AS NUMPY
COMPUTED IT (the blend takes the divisor as an input), top_k, n_items, and the reference's answer: `ids` and `values`.  A case is a
list in the order of `case_fields`; id lists (int16), float32 lists (and the norm) and the float64 answers are stored as base64 of
their little-endian bytes, one string per list, so that every bit survives and the file stays small.  Three conditions are asserted and recorded:
  share_an_item >= 100                 fixture queries with an item in both lists
  value_not_float32 >= 50              fixture queries that return a value which is not a float32 number
  order_float32_would_change >= 1      cases whose order a float32 comb_sum would change

    python tools/gen_golden_similar.py
"""
import base64
import json
import os
import struct
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_SMALL, SMALL_ITEMS = 60, 24
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


class Script:
    """What the stand-ins answer for the case being run."""
    vectors = None          # (biases [n], embeddings [n, d]) of all items
    query = 0
    a_list = None           # (ids, s1) the top-k returns, or None: computed by the host model
    b_list = None           # (ids, float32 scores) slim_model.similar_items returns
    seen = None             # what the top-k was handed and returned


def make_instance(hybrid_cls, script):
    inst = hybrid_cls.__new__(hybrid_cls)
    inst.use_bias = True
    inst.n_threads = 1
    inst._create_item_features = lambda item_ids=None, items_tags=None, slice=False: ("query", item_ids[0]) if item_ids is not None else "all"

    def representations(features):
        b, e = script.vectors
        if features == "all":
            return b, e
        q = features[1]
        return b[q:q + 1], e[q:q + 1]

    inst.model = types.SimpleNamespace(get_item_representations=representations)
    inst.slim_model = types.SimpleNamespace(similar_items=lambda q, top_k=10, ret_ndarrays=False: script.b_list)
    return inst


def main() -> int:
    from ref_import import import_reference
    import_reference()
    import rtrec.models.hybrid as H
    from tests.test_explain_host import golden
    from tests.test_similar_host import (blend_row_fast, blend_row_plain, host_similar_fast, host_slim_similar, lists_of, order_case)

    script = Script()

    def topk(items, query, k, item_norms=None, filter_items=None, num_threads=0, **kw):
        assert query.shape[0] == 1 and filter_items is not None and len(filter_items) == 1
        if script.a_list is not None:
            ids, s1 = script.a_list
        else:
            out = host_similar_fast(items, item_norms, [int(filter_items[0])], k, P=query, p_norms=np.ones(1, F32))
            n = int(out[2][0])
            ids, s1 = out[0][0, :n].astype(np.int64), out[1][0, :n]
        script.seen = (np.array(ids), np.array(s1, F32))
        return np.array(ids, np.int32)[None, :], np.array(s1, F32)[None, :]

    H.implicit.topk = topk
    inst = make_instance(H.HybridSlimFM, script)

    _, W, _, _, _ = golden()
    W = W.tocsc().astype(F32)
    n_items = int(W.shape[1])
    assert n_items == 400 and (np.diff(W.indptr) > 0).all()
    rng = np.random.default_rng(20261019)
    S = (W + W.T).toarray().astype(np.float64)
    u, s, _ = np.linalg.svd(S)
    emb = (u[:, :11] * np.sqrt(s[:11])[None, :] + 0.02 * rng.standard_normal((n_items, 11))).astype(F32)
    bias = (0.1 * rng.standard_normal(n_items)).astype(F32)
    f32 = lambda a: [float(v) for v in np.asarray(a, dtype=F32)]
    b64 = lambda a, dt: base64.b64encode(np.asarray(a, dtype=dt).tobytes()).decode()       # how the file stores its lists
    cases = []

    def run(q, top_k, n):
        script.query = q
        answer = inst._similar_items(q, None, top_k)
        b, e = script.vectors
        qv = np.hstack((b[q:q + 1, np.newaxis], e[q:q + 1]), dtype=np.float32)
        norm = H.calc_norm(qv)
        assert norm.dtype == np.float32 and norm.shape == (1,)
        a_ids, a_s1 = script.seen
        assert all(isinstance(v, float) for _, v in answer)
        return dict(n_items=n, query=int(q), query_norm=float(norm[0]), top_k=int(top_k), a_ids=[int(i) for i in a_ids], a_scores=f32(a_s1),
                    b_ids=[int(i) for i in script.b_list[0]], b_scores=f32(script.b_list[1]), ids=[int(i) for i, _ in answer],
                    value_hex=[struct.pack("<d", v).hex() for _, v in answer])

    script.vectors = (bias, emb)
    for q in range(n_items):
        script.a_list = None
        script.b_list = host_slim_similar(W, q, 10)
        cases.append(run(q, 10, n_items))

    n_order, A, B = order_case()
    for c in range(N_SMALL):
        q = int(rng.integers(0, SMALL_ITEMS))
        script.vectors = ((0.1 * rng.standard_normal(SMALL_ITEMS)).astype(F32),
                          (rng.standard_normal((SMALL_ITEMS, 5)) * (1e-3, 1.0, 40.0)[c % 3]).astype(F32))
        if c == 0:
            la, lb = int(A[2][0]), int(B[2][0])
            script.a_list = (A[0][0, :la].astype(np.int64), A[1][0, :la])
            script.b_list = (B[0][0, :lb].astype(np.int64), B[1][0, :lb])
            q = 20
        else:
            la, lb = int(rng.integers(1, 13)), int(rng.integers(1, 13))
            scale = (1.0, 1e-9, 50.0)[c % 3]
            a_ids = rng.integers(0, SMALL_ITEMS, la)
            if (a_ids == q).all():
                a_ids[0] = (q + 1) % SMALL_ITEMS
            if c % 4 == 1 and a_ids[0] != q:                  # the query inside A, behind the head
                a_ids = np.r_[a_ids, q]
            a_sc = np.full(len(a_ids), rng.random(), F32) if c % 5 == 0 else -np.sort(-rng.standard_normal(len(a_ids)).astype(F32))
            a_sc = (a_sc * F32(scale)).astype(F32)
            if c % 6 == 2:                                    # implicit's marker for what it filtered out ends the list
                a_ids, a_sc = np.r_[a_ids, rng.integers(0, SMALL_ITEMS, 2)], np.r_[a_sc, F32(-FLT_MAX), F32(-FLT_MAX)].astype(F32)
            b_ids = rng.integers(0, SMALL_ITEMS - 1, lb)
            b_ids = np.where(b_ids >= q, b_ids + 1, b_ids)    # SLIM's list never holds the query
            b_sc = np.full(lb, rng.random(), F32) if c % 5 == 1 else -np.sort(-rng.standard_normal(lb).astype(F32))
            script.a_list = (a_ids.astype(np.int64), a_sc)
            script.b_list = (b_ids.astype(np.int64), (b_sc * F32(scale)).astype(F32))
        top_k = int(rng.integers(1, len(script.a_list[0]) + len(script.b_list[0]) + 1)) if c else 6
        cases.append(run(q, top_k, SMALL_ITEMS))

    # both host models must give the reference's answer, and the three conditions
    share = wide = order32 = 0
    for n, c in enumerate(cases):
        A1, B1 = lists_of([c["a_ids"]], [c["a_scores"]]), lists_of([c["b_ids"]], [c["b_scores"]])
        rows = {}
        for fn in (blend_row_plain, blend_row_fast):
            rows[fn] = fn(c["n_items"], A1[0][0], A1[1][0], A1[2][0], F32(c["query_norm"]), B1[0][0], B1[1][0], B1[2][0], c["query"])[:c["top_k"]]
            assert [i for i, _, _ in rows[fn]] == c["ids"], (n, fn.__name__, "ids")
            assert [struct.pack("<d", float(v)).hex() for _, v, _ in rows[fn]] == c["value_hex"], (n, fn.__name__, "values")
        r32 = blend_row_fast(c["n_items"], A1[0][0], A1[1][0], A1[2][0], F32(c["query_norm"]), B1[0][0], B1[1][0], B1[2][0], c["query"],
                             sum_dtype=np.float32)[:c["top_k"]]
        order32 += [i for i, _, _ in r32] != c["ids"]
        if n < n_items:
            share += bool(set(c["a_ids"]) & set(c["b_ids"]))
            wide += any(float(F32(v)) != float(v) for _, v, _ in rows[blend_row_fast])
    conditions = dict(share_an_item=int(share), value_not_float32=int(wide), order_float32_would_change=int(order32))
    assert share >= 100 and wide >= 50 and order32 >= 1, conditions
    repeated = sum(len(set(c["a_ids"])) < len(c["a_ids"]) or len(set(c["b_ids"])) < len(c["b_ids"]) for c in cases[n_items:])
    out = dict(numpy_version=np.__version__, n_fixture=n_items, n_small=N_SMALL, small_cases_with_repeated_ids=int(repeated),
               conditions=conditions,
               case_fields=["n_items", "query", "query_norm", "top_k", "a_ids", "a_scores", "b_ids", "b_scores", "ids", "values"],
               cases=[[c["n_items"], c["query"], b64(c["query_norm"], "<f4"), c["top_k"], b64(c["a_ids"], "<i2"), b64(c["a_scores"], "<f4"),
                       b64(c["b_ids"], "<i2"), b64(c["b_scores"], "<f4"), b64(c["ids"], "<i2"), base64.b64encode(bytes.fromhex("".join(c["value_hex"]))).decode()] for c in cases])
    path = os.path.join(ROOT, "tests", "golden", "similar_blend.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print(json.dumps({k: v for k, v in out.items() if k != "cases"}), os.path.getsize(path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
