#!/usr/bin/env python3
"""Writes tests/golden/blend.json: what the reference's HybridSlimFM._ensemble_by_scores answers for seeded pairs of lists.

Runs only where the reference is installed beside this repository (tools/ref_import.py); no test imports this file.  The
method is called on an instance made WITHOUT its constructor (the constructor builds the LightFM half, which is not installed
and not needed): the instance gets the reference's own interaction store, an empty interaction_counts dict and
similarity_weight_factor = k, and the contacts are entered the way the hybrid's fit enters them -- add_interaction, then
_incr_interaction_counts once per further contact.

Cases, in this order:
  * the 240 fixture users of tests/golden/scoring.npz: B = the recorded reference top-10 (ids and float32 scores), A = a seeded
    list of 10 that shares about half its items with B, seeded contact counts 1..5 on about 40 % of B's items; k alternates
    between 2.0 and 0.5;
  * 60 small seeded cases over 24 items: lengths 1..12, ids drawn WITH replacement (repeated ids in either list), every fifth
    list with all scores equal, scores scaled by 1e-9 and by 50 in turn, contacts on about half the items.

Per case the file holds both lists, the items the user's row stores (`x_items`: one contact or more), the counts of two or more
(`counts`: what interaction_counts holds), k, and `ids`: the reference's answer for top_k = the whole union.  Three conditions on
the 240 user cases are asserted and recorded (they make the fixture worth having; the host model of tests/test_blend_host.py
supplies the values the reference does not return):
  order_differs_from_a >= 100        the blended top-10 is not A's list
  tie_decided_by_position >= 100     two entries of the blended list (the whole union, which `ids` records) have == values
  lists_an_item_only_b_holds >= 50   the blended top-10 shows an item A does not hold

    python tools/gen_golden_blend.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_SMALL, SMALL_ITEMS = 60, 24


def reference_answer(hybrid_cls, store_cls, user, case, top_k):
    inst = hybrid_cls.__new__(hybrid_cls)
    inst.interactions = store_cls(min_value=0, max_value=15)
    inst.interaction_counts = {}
    inst.similarity_weight_factor = float(case["k"])
    for item, n in case["contacts"]:
        inst.interactions.add_interaction(user, item, 1.7e9, 1.0)
        for _ in range(n - 1):
            inst._incr_interaction_counts(user, item)
    out = inst._ensemble_by_scores(user, np.array(case["a_ids"], np.int64), np.array(case["a_scores"], np.float32),
                                   [int(i) for i in case["b_ids"]], np.array(case["b_scores"], np.float32), top_k)
    return [int(i) for i in out]


def main() -> int:
    from ref_import import import_reference
    import_reference()
    from rtrec.models.hybrid import HybridSlimFM
    from rtrec.utils.interactions import UserItemInteractions
    from tests.test_blend_host import csr_of_rows, host_model, pad_lists
    from tests.test_explain_host import golden

    X, W, users, ref_ids, ref_scores = golden()
    n_items = int(W.shape[1])
    rng = np.random.default_rng(20261019)
    f32 = lambda a: [float(v) for v in np.asarray(a, dtype=np.float32)]
    cases = []
    for b, u in enumerate(users.tolist()):
        b_ids = [int(i) for i in ref_ids[b]]
        shared = rng.permutation(10)[:int(rng.integers(4, 7))]
        others = [int(i) for i in rng.permutation(n_items) if int(i) not in b_ids][:10 - len(shared)]
        a_ids = [b_ids[j] for j in shared] + others
        a_ids = [a_ids[j] for j in rng.permutation(10)]
        a_scores = -np.sort(-(rng.random(10) * 4.0 - 1.0).astype(np.float32))
        contacts = [[b_ids[j], int(rng.integers(1, 6))] for j in range(10) if rng.random() < 0.4]
        cases.append(dict(user=int(u), a_ids=a_ids, a_scores=f32(a_scores), b_ids=b_ids, b_scores=f32(ref_scores[b]),
                          contacts=contacts, k=2.0 if b % 2 == 0 else 0.5))
    for c in range(N_SMALL):
        la, lb = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        scale = (1.0, 1e-9, 50.0)[c % 3]
        lists = []
        for n, flat in ((la, c % 5 == 0), (lb, c % 5 == 1)):
            ids = [int(i) for i in rng.integers(0, SMALL_ITEMS, n)]
            sc = np.full(n, rng.random(), np.float32) if flat else -np.sort(-rng.standard_normal(n).astype(np.float32))
            lists.append((ids, f32(sc * np.float32(scale))))
        contacts = [[i, int(rng.integers(1, 6))] for i in range(SMALL_ITEMS) if rng.random() < 0.5]
        cases.append(dict(user=1000 + c, a_ids=lists[0][0], a_scores=lists[0][1], b_ids=lists[1][0], b_scores=lists[1][1],
                          contacts=contacts, k=2.0 if c % 2 == 0 else 0.5))
    for case in cases:
        case["ids"] = reference_answer(HybridSlimFM, UserItemInteractions, case["user"], case, len(case["a_ids"]) + len(case["b_ids"]))
        case["x_items"] = sorted(i for i, _ in case["contacts"])
        case["counts"] = sorted([i, n] for i, n in case["contacts"] if n >= 2)
        del case["contacts"]

    # the three conditions, on the user cases
    U = len(users)
    differs = ties_n = b_only = 0
    for r, case in enumerate(cases[:U]):
        A = (pad_lists([case["a_ids"]])[0], pad_lists([case["a_scores"]], None, 0.0, np.float32)[0], [len(case["a_ids"])])
        B = (pad_lists([case["b_ids"]])[0], pad_lists([case["b_scores"]], None, 0.0, np.float32)[0], [len(case["b_ids"])])
        counted = {int(i): n for i, n in case["counts"]}
        con = dict(X=csr_of_rows([case["x_items"]], n_items), C=csr_of_rows([list(counted)], n_items, [counted]), rows=None)
        ties = []
        whole = host_model(n_items, A, B, 20, contacts=con, k=case["k"], ties=ties)
        assert whole[0][0, :whole[3][0]].tolist() == case["ids"], f"user case {r}: the host model and the reference disagree"
        ids, value, source, count = host_model(n_items, A, B, 10, contacts=con, k=case["k"])
        assert ids[0, :count[0]].tolist() == case["ids"][:10]
        differs += ids[0].tolist() != case["a_ids"]
        ties_n += bool(ties)
        b_only += bool((source[0, :count[0]] == 2).any())
    conditions = dict(order_differs_from_a=int(differs), tie_decided_by_position=int(ties_n), lists_an_item_only_b_holds=int(b_only))
    assert differs >= 100 and ties_n >= 100 and b_only >= 50, conditions
    repeated = sum(len(set(c["a_ids"])) < len(c["a_ids"]) or len(set(c["b_ids"])) < len(c["b_ids"]) for c in cases[U:])
    out = dict(numpy_version=np.__version__, n_items=n_items, n_users=U, n_small=N_SMALL, small_cases_with_repeated_ids=int(repeated),
               conditions=conditions, cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "blend.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print(json.dumps({k: v for k, v in out.items() if k != "cases"}), os.path.getsize(path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
