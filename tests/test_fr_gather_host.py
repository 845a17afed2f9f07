"""Where score_frows_kernel cuts W into the resident head and the gathered rest -- the host side of it.

rtrec_slim_score_fr_lds_bytes is the launch code's own plan (csrc/score.hip, fr_lds_plan): how many KiB of LDS the head
gets and what every wave keeps as setup scratch / row ring.  The kernel then keeps the leading super-tiles that fit.
No GPU: the plan is a pure host function of the library, and it is the only library code these tests run.  The cut itself
is made in the kernel, from tables in device memory: `head_cut` below is a Python MODEL of that rule, used here to check
that the layouts and head sizes of tests/test_gpu_fr_gather.py are the boundaries they claim to be.  An off-by-one in the
kernel's own cut is caught only by the GPU tests there (a head that ends between tiles, inside a tile, in front of the
last super-tile)."""
import ctypes as C

import numpy as np
import pytest

from rtrec_amd import _native

from .test_gpu_fr_gather import grouped_w, head_cuts, host_layout

LDS_CU = 160 * 1024
WAVES, RING_BYTES, EXTRA = 16, 4096, 16 * 576 + 1024 + 16


def plan(n_super, n_tiles, tc, n_frags, buf_bytes, cap=-1):
    L = _native.load()
    head, scratch = C.c_int32(-1), C.c_int32(-1)
    lds = L.rtrec_slim_score_fr_lds_bytes(n_super, n_tiles, tc, n_frags, buf_bytes, cap, C.byref(head), C.byref(scratch))
    return int(lds), head.value, scratch.value


def plan_of(L, cap=-1):
    return plan(L["fr_n_super"], L["fr_n_tiles"], L["fr_tile_cols"], L["fr_n_frags"], L["fr_buf_bytes"], cap)


def head_cut(L, head_kib):
    """(super-tiles, fragments) of the head: the largest S with kb[S] - kb[0] <= head_kib, and its first fragment."""
    kb, st = np.asarray(L["fr_super_kb"]), np.asarray(L["fr_super_tile"])
    s = 0
    while s < L["fr_n_super"] and kb[s + 1] - kb[0] <= head_kib:
        s += 1
    return s, int(st[s])


def test_ml20m_shape_keeps_two_super_tiles():
    """28 super-tiles of 36 KiB, 104 tiles, 130 fragments: 4 KiB per wave for the ring, 85 KiB for the head."""
    lds, head, scratch = plan(28, 104, 256, 130, 36 * 1024)
    assert scratch == RING_BYTES and head == 85 and lds <= LDS_CU
    assert lds == head * 1024 + WAVES * scratch + EXTRA + 4 * 130 + 8          # (the suffix bounds round up to 16 bytes)
    L = dict(fr_super_kb=np.arange(29) * 36, fr_super_tile=np.arange(29) * 4, fr_n_super=28)
    assert head_cut(L, head) == (2, 8)


def test_resident_w_is_all_head_with_the_small_scratch():
    """One super-tile that fits beside the scratch its masks need: today's resident form, nothing to gather."""
    for n_tiles, buf_kib in ((4, 60), (24, 100), (64, 80)):
        lds, head, scratch = plan(1, n_tiles, 256, n_tiles, buf_kib * 1024)
        assert head == buf_kib and lds <= LDS_CU
        assert scratch == -(-(n_tiles * 4 * 8 + 768) // 256) * 256 <= RING_BYTES
    # ... too large for that: the ring's 4 KiB per wave, and the kernel finds no super-tile that fits the head
    lds, head, scratch = plan(1, 24, 256, 24, 130 * 1024)
    assert scratch == RING_BYTES and head < 130 and lds <= LDS_CU


def test_all_resident_agrees_with_the_layout_builder():
    """layouts.py calls a W resident (one super-tile, strided work order) by a formula that knows no table of suffix
    bounds.  The plan must not disagree about a W that fits only without the table: such a one-super-tile W would fit no
    head and every row of it would be gathered.  It stays all resident; the launch then reserves no table."""
    n_tiles, n_frags = 64, 64
    setup = -(-(n_tiles * 4 * 8 + 768) // 256) * 256
    fixed = WAVES * setup + EXTRA
    buf = (LDS_CU - fixed) // 1024 * 1024                       # the largest W that fits without the table
    lds, head, scratch = plan(1, n_tiles, 256, n_frags, buf)
    assert head == buf >> 10 and scratch == setup and lds <= LDS_CU
    assert lds in (buf + fixed, buf + fixed + 4 * n_frags)
    if LDS_CU - (buf + fixed) < 4 * n_frags:                    # (the window: no room for the table)
        assert lds == buf + fixed
    lds, head, scratch = plan(1, n_tiles, 256, n_frags, buf - 1024)
    assert head == (buf >> 10) - 1 and lds == buf - 1024 + fixed + 4 * n_frags
    assert plan(1, n_tiles, 256, n_frags, buf + 1024)[2] == RING_BYTES


def test_flat_w_of_several_super_tiles_fits_the_head():
    """More than 64 narrow tiles in 70 / 79 KiB (the flat cases of the GPU tests): the head is capped at W's size, or is
    what the LDS leaves; either way the model cut keeps every super-tile, and the cap `all but the last` keeps all but it."""
    from .test_gpu_fr_gather import FLAT
    for name, spec in FLAT.items():
        W, _, _ = grouped_w(50, seed=len(name) + 50 * len(spec), spec=spec)
        L = host_layout(W, 128)
        kb = np.asarray(L["fr_super_kb"])
        lds, head, scratch = plan_of(L)
        w_kib = L["fr_n_super"] * (L["fr_buf_bytes"] >> 10)
        assert scratch == RING_BYTES and lds <= LDS_CU and head == min(w_kib, 85) and head >= kb[-1] - kb[0]
        assert head_cut(L, head)[0] == L["fr_n_super"]
        cap = int(kb[-2] - kb[0])
        assert plan_of(L, cap)[1] == cap and head_cut(L, cap) == (L["fr_n_super"] - 1, int(np.asarray(L["fr_super_tile"])[-2]))


def test_a_cap_never_grows_the_head_and_always_leaves_a_ring():
    for shape in ((28, 104, 256, 130, 36 * 1024), (1, 4, 256, 4, 60 * 1024), (3, 70, 128, 80, 36 * 1024)):
        _, free_head, _ = plan(*shape)
        last = -1
        for cap in (0, 1, 35, 36, 37, 72, 84, 126):
            lds, head, scratch = plan(*shape, cap)
            assert lds <= LDS_CU and head <= free_head and head >= last
            assert head == min(cap, free_head) or (shape[0] == 1 and head == free_head)
            if head < shape[0] * (shape[4] >> 10):              # something is gathered: the wave's scratch holds the ring
                assert scratch >= RING_BYTES
            last = head
        assert plan(*shape, 0)[1] == 0


def test_layouts_the_kernel_does_not_take():
    assert plan(0, 4, 256, 4, 36 * 1024)[0] == 0
    assert plan(2, 4, 192, 4, 36 * 1024)[0] == 0
    assert plan(2, 4, 256, 3, 36 * 1024)[0] == 0                # fewer fragments than tiles
    assert plan(2, 4, 256, 4, 36 * 1024 + 512)[0] == 0
    assert plan(2, 105, 256, 105, 36 * 1024)[0] == 0            # more mask words than the setup scratch holds


@pytest.mark.parametrize("n_feat,tc", [(110, 256), (110, 128), (50, 256), (50, 128)])
def test_head_cut_on_real_layouts(n_feat, tc):
    """The head ends between super-tiles: every fragment in front of the cut lies inside the head's bytes, the first one
    behind it does not fit; the cuts the GPU tests use are the tile / inside-a-tile boundaries they claim to be."""
    W, _, _ = grouped_w(n_feat, seed=n_feat)
    L = host_layout(W, tc)
    kb, st, ft, off = (np.asarray(L[k]) for k in ("fr_super_kb", "fr_super_tile", "fr_frag_tile", "fr_tile_off"))
    rows = np.array([bin(int(a)).count("1") + bin(int(b)).count("1")
                     for a, b in np.asarray(L["fr_tile_rows"]).view(np.uint64).reshape(-1, 2)])
    sup_of = np.searchsorted(st, np.arange(L["fr_n_frags"]), side="right") - 1
    end = (kb[sup_of] - kb[0]) * 1024 + off + rows * tc * 4    # byte behind fragment g in W's image
    _, free_head, scratch = plan_of(L)
    assert scratch == RING_BYTES and L["fr_n_super"] > 1
    for head in sorted({0, 1, free_head, *[v for v in head_cuts(L).values() if v is not None]}):
        s, g = head_cut(L, head)
        assert (end[:g] <= head * 1024).all()
        assert s == L["fr_n_super"] or kb[s + 1] - kb[0] > head
        assert plan_of(L, head)[1] == min(head, free_head)
    cuts = head_cuts(L)
    s, g = head_cut(L, cuts["inside"])
    assert s >= 1 and not ft[g] & (1 << 24) and (ft[g - 1] & 0xFFFFFF) == (ft[g] & 0xFFFFFF)     # the tile continues behind the cut
    if cuts["between"] is not None:
        s, g = head_cut(L, cuts["between"])
        assert ft[g] & (1 << 24) and ft[g - 1] & (1 << 25)
    assert head_cut(L, 0) == (0, 0)
    assert head_cut(L, free_head)[0] == int(np.searchsorted(kb - kb[0], free_head, side="right")) - 1
