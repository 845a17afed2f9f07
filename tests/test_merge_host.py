"""Host checks that go with tests/test_gpu_merge.py: the record layout of the column-sharded exchange, and the agreement of
that module's numpy model of the merge with the stand-in backend's (tests/cpu_backend.py) on the very inputs the GPU tests use."""
import itertools

import numpy as np
import pytest

from rtrec_amd.engine import exchange_record_layout, exchange_record_views
from tests import test_gpu_merge as tm


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("k", [1, 10, 63, 64])
def test_exchange_record_layout(k, f64):
    L = exchange_record_layout(k, f64)
    # exchanged record: [float64 scores]? | scores | ids | aux | count | pad -- blocks in this order, back to back, no overlap
    blocks = ([("sc64", 0, 2 * k)] if f64 else []) + [("sc", L["o_sc"], k), ("ids", L["o_ids"], k), ("aux", L["o_aux"], k),
                                                      ("cnt", L["o_cnt"], 1)]
    at = 0
    for name, off, n in blocks:
        assert off == at, f"{name} starts at {off}, the block before it ends at {at}"
        at = off + n
    assert L["width"] % 2 == 0 and L["fwidth"] % 2 == 0
    assert L["o_cnt"] + 1 <= L["width"] <= L["o_cnt"] + 2          # the count is the last word before at most one pad word
    # a float64 block starts every record, and records are a whole number of doubles: 8-byte aligned in an aligned buffer
    assert not f64 or (blocks[0][1] == 0 and (L["width"] * 4) % 8 == 0)
    # final record: scores | ids | count | pad
    assert (L["f_ids"], L["f_cnt"]) == (k, 2 * k) and L["f_cnt"] + 1 <= L["fwidth"] <= L["f_cnt"] + 2


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_exchange_record_views_address_the_layout(f64):
    """Every word of a record buffer is addressed by exactly one view entry (the float64 block by one double per two words),
    except the pad word."""
    import torch
    G, q, k = 3, 5, 7
    L = exchange_record_layout(k, f64)
    recv = torch.zeros((G * q, L["width"]), dtype=torch.int32)
    ids, sc, sc64, aux, cnt = exchange_record_views(torch, recv, G, q, k, f64)
    assert ids.shape == sc.shape == aux.shape == (G, q, k) and cnt.shape == (G, q)
    assert sc.dtype == torch.float32 and (sc64 is None) == (not f64)
    ids += 1; aux += 1; cnt += 1
    sc.view(torch.int32).add_(1)
    if f64:
        assert sc64.shape == (G, q, k) and sc64.dtype == torch.float64
        sc64.view(torch.int64).add_((1 << 32) + 1)
    hit = recv.numpy()
    assert (hit[:, :L["o_cnt"] + 1] == 1).all() and (hit[:, L["o_cnt"] + 1:] == 0).all()
    # [source shard, row, entry]: list l, row u is record l * q + u
    ids[2, 1, 3] = 99
    assert hit[2 * q + 1, L["o_ids"] + 3] == 99


CASES = [(l, k, f, 257, 0) for (l, k), f in itertools.product(tm.MERGE_CASES, (False, True))] + \
        [(G, k, f, tm.EXCHANGE_Q, 3) for G, k, f in itertools.product((2, 3, 8), (10, 50), (False, True))]


@pytest.mark.parametrize("n_lists,top_k,f64,n_rows,pad_rows", CASES,
                         ids=[f"{tm.case_id(c[0], c[1])}-{'f64' if c[2] else 'f32'}-{c[3]}rows" for c in CASES])
def test_merge_model_agrees_with_the_stand_in_backend(n_lists, top_k, f64, n_rows, pad_rows):
    import torch
    from tests.cpu_backend import OracleBackend
    ids, sc, sc64, aux, cnt = tm.make_lists(n_lists, top_k, f64, n_rows, pad_rows)
    # the inputs are inside the precondition of the merge: ids distinct across the lists of a row, no NaN
    valid = np.arange(top_k)[None, None, :] < cnt[:, :, None]
    for r in range(n_rows):
        v = ids[:, r, :][valid[:, r, :]]
        assert len(np.unique(v)) == len(v)
    assert not np.isnan(sc).any()
    if f64:
        assert np.array_equal(sc, sc64.astype(np.float32)) and (sc64[valid] != sc[valid]).any()
    t = [torch.from_numpy(np.array(a)) if a is not None else None for a in (ids, sc, sc64, aux.view(np.int32), cnt)]
    o_ids = torch.empty((n_rows, top_k), dtype=torch.int32)
    o_sc = torch.empty((n_rows, top_k), dtype=torch.float32)
    o_cnt = torch.empty((n_rows,), dtype=torch.int32)
    OracleBackend().merge_topk(n_rows, n_lists, top_k, *t, o_ids, o_sc, o_cnt)
    tm.assert_lists_equal((o_ids.numpy(), o_sc.numpy(), o_cnt.numpy()), tm.expected(n_lists, top_k, f64, n_rows, pad_rows),
                          "stand-in backend vs numpy model")
