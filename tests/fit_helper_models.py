"""Plain numpy models and input builders of the fit-side helper kernels and of the segment-layout builder.  TEST-ONLY.

Shared by tests/test_fit_helpers_host.py (holds the models to the C oracle and to the numpy specification, on the CPU) and
tests/test_gpu_fit_helpers.py (holds the kernels to the models).  Four parts:

  A  the one-pass X^T y of a small fit call (csrc/fit.hip: xty_tmap_kernel, xty_compact_kernel, xty_batch_kernel), read
     from its own scratch: a mirror of the scratch layout, the compacted rows, the per-target lists of non-zero sums;
  B  the matrix of the slot-reuse tests;
  C  column norms and the Gram matrix at the boundaries their loops branch on;
  D  constructed W shards for csrc/seg_build.hip and a decoder of the segment layout that shares no code with
     seg_layout.build_seg_layout.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Tuple

import numpy as np
import scipy.sparse as sp

from rtrec_amd.synth import interaction_matrix


def f32_bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def both_orientations(X) -> Tuple[sp.csc_matrix, sp.csr_matrix]:
    """(CSC, CSR) with sorted indices, float32, stored zeros removed."""
    Xr = sp.csr_matrix(X, dtype=np.float32)
    Xr.eliminate_zeros()
    Xr.sort_indices()
    Xc = Xr.tocsc()
    Xc.sort_indices()
    return Xc, Xr


# ------------------------------------------------------------------------------------------------ A: one-pass X^T y
XTY_MAX_TARGETS = 2048          # kXtyMaxTargets of csrc/fit.hip


def xty_model(Xr: sp.csr_matrix, targets: np.ndarray) -> np.ndarray:
    """S[g, i] = s_t[i] for t = targets[g]: start from +0.0f, users ascending, every step adds fl32(X[u, i] * X[u, t]) and
    rounds once; S[g, t] = 0 (the target's own column is masked).  The dense loop: an absent X[u, i] adds +0, which changes no
    sum (a sum that starts from +0 never becomes -0)."""
    D = Xr.toarray().astype(np.float32)
    Xc = Xr.tocsc()
    Xc.sort_indices()
    S = np.zeros((len(targets), Xr.shape[1]), dtype=np.float32)
    for g, t in enumerate(np.asarray(targets).tolist()):
        s = S[g]
        for u in Xc.indices[Xc.indptr[t]:Xc.indptr[t + 1]].tolist():
            s += (D[u] * D[u, t]).astype(np.float32)
        s[t] = 0.0
    return S


def xty_lists(S: np.ndarray) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Per target the expected candidate list {(i, s_t[i]) : s_t[i] != 0}, ascending item id."""
    out = []
    for g in range(S.shape[0]):
        ids = np.flatnonzero(S[g] != 0)
        out.append((ids.astype(np.int32), S[g, ids].copy()))
    return out


def xty_ws_mirror(n_users: int, n_items: int, nnz: int, n_t: int) -> Dict[str, int]:
    """Byte offsets of the one-pass X^T y scratch (xty_ws_layout of csrc/fit.hip), every field rounded up to 256 bytes, and
    `total` -- which must equal rtrec_slim_xty_workspace_bytes."""
    up = lambda v: -(-v // 256) * 256
    L, o = {}, 0
    for name, nbytes in (("tmap", 4 * n_items), ("ypos", 4 * n_users), ("ylen", 4 * n_users), ("cursor", 256), ("cand_cnt", 4 * n_t),
                         ("yt", 4 * nnz), ("yv", 4 * nnz), ("cand_i", 4 * n_t * n_items), ("cand_s", 4 * n_t * n_items)):
        L[name] = o
        o = up(o + nbytes)
    L["total"] = o
    return L


def xty_compact_model(Xr: sp.csr_matrix, targets: np.ndarray) -> Tuple[np.ndarray, List[Tuple[np.ndarray, np.ndarray]]]:
    """(tmap[I], per user (target indices, values)): a user's stored entries restricted to the call's targets, in stored
    order, items mapped to their position in `targets`."""
    tmap = np.full(Xr.shape[1], -1, dtype=np.int32)
    tmap[np.asarray(targets)] = np.arange(len(targets), dtype=np.int32)
    per_user = []
    for u in range(Xr.shape[0]):
        c = Xr.indices[Xr.indptr[u]:Xr.indptr[u + 1]]
        v = Xr.data[Xr.indptr[u]:Xr.indptr[u + 1]]
        keep = tmap[c] >= 0
        per_user.append((tmap[c[keep]], v[keep].astype(np.float32)))
    return tmap, per_user


def targets_per_user(Xr: sp.csr_matrix, targets: np.ndarray) -> np.ndarray:
    """How many of the call's targets every user has rated (the kernel's `len`; its tail loop runs from 65)."""
    is_t = np.zeros(Xr.shape[1], dtype=np.int64)
    is_t[np.asarray(targets)] = 1
    return np.asarray(Xr.astype(bool).astype(np.int64) @ is_t).ravel()


@dataclass(frozen=True)
class XtyCase:
    X: sp.csr_matrix            # U x I, float32, sorted indices
    targets: np.ndarray         # in exactly the order of the call
    K: int
    positive: bool
    notes: Dict[str, int]       # items a test looks at by name


def _shuffled_targets(n_items: int, n: int) -> np.ndarray:
    return np.random.default_rng(3).permutation(n_items)[:n].astype(np.int64)


@functools.lru_cache(maxsize=None)
def _xty_base() -> sp.csr_matrix:
    return both_orientations(interaction_matrix(700, 300, 40000, seed=7))[1]


@functools.lru_cache(maxsize=None)
def _xty_subset_matrix() -> Tuple[sp.csr_matrix, int, int]:
    """The base matrix with one target column emptied and one target column cut down to its first user."""
    tg = _shuffled_targets(300, 200)
    empty, single = int(tg[5]), int(tg[17])
    X = _xty_base().tolil()
    X[:, empty] = 0
    users = _xty_base().tocsc()[:, single].indices
    assert len(users) > 1
    X[np.sort(users)[1:], single] = 0
    return both_orientations(X.tocsr())[1], empty, single


@functools.lru_cache(maxsize=None)
def xty_case(name: str) -> XtyCase:
    """The inputs of part A by name: all_ascending | subset_shuffled | nt1 | nt64 | nt65 | cap2048 | signed | denormal."""
    if name == "all_ascending":
        return XtyCase(_xty_base(), np.arange(300, dtype=np.int64), 10, True, {})
    if name in ("subset_shuffled", "denormal"):
        X, empty, single = _xty_subset_matrix()
        if name == "denormal":          # ratings of ~2^-70: every product and every sum is a denormal float32 (or zero)
            X = X.copy()
            X.data = (X.data * np.float32(2.0 ** -70)).astype(np.float32)
        return XtyCase(X, _shuffled_targets(300, 200), 10, True, {"empty": empty, "single": single})
    if name in ("nt1", "nt64", "nt65"):
        return XtyCase(_xty_base(), _shuffled_targets(300, int(name[2:])), 10, True, {})
    if name == "cap2048":
        X = both_orientations(interaction_matrix(300, 2100, 42000, seed=7))[1]
        return XtyCase(X, _shuffled_targets(2100, XTY_MAX_TARGETS), 10, True, {})
    if name == "signed":
        # signs as tests/test_gpu_kernels.py::test_fit_with_negative_ratings_bit_exact draws them, plus one planted pair:
        # feature column (1, 1) against target column (2, -2) on the same two users -- the two products cancel to exactly 0
        X = _xty_base().copy()
        rng = np.random.default_rng(5)
        X.data = (X.data * np.where(rng.random(X.nnz) < 0.25, -1.0, 1.0)).astype(np.float32)
        perm = np.random.default_rng(3).permutation(300)
        target, feature = int(perm[0]), int(perm[250])
        X = X.tolil()
        X[:, target] = 0
        X[:, feature] = 0
        X[11, feature], X[402, feature] = 1.0, 1.0
        X[11, target], X[402, target] = 2.0, -2.0
        return XtyCase(both_orientations(X.tocsr())[1], perm[:200].astype(np.int64), 10, False,
                       {"target": target, "feature": feature})
    raise KeyError(name)


XTY_CASES = ("all_ascending", "subset_shuffled", "nt1", "nt64", "nt65", "cap2048", "signed", "denormal")


# ------------------------------------------------------------------------------------------------ B: slot reuse
@functools.lru_cache(maxsize=None)
def slot_matrix(signed: bool = False) -> Tuple[sp.csc_matrix, sp.csr_matrix]:
    """interaction_matrix(600, 200, 12000, seed=11) in both orientations; signed: a quarter of the ratings negated."""
    X = interaction_matrix(600, 200, 12000, seed=11)
    if signed:
        rng = np.random.default_rng(5)
        X.data = (X.data * np.where(rng.random(X.nnz) < 0.25, -1.0, 1.0)).astype(np.float32)
    return both_orientations(X)


# ------------------------------------------------------------------------------------------------ C: norms and Gram matrix
SQN_HEAD_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000, 4097)
SQN_N_ITEMS = 8192 + 37         # the launch's grid is capped at 8,192 workgroups: the last 37 columns come from the stride loop
SQN_INF_COLUMN = 12             # the 1000-entry column holds ten values of 1e19: its running sum reaches inf


def sqnorm_model(cptr: np.ndarray, cval: np.ndarray) -> np.ndarray:
    """acc = float32(acc + float32(v * v)), left to right, per column."""
    out = np.zeros(len(cptr) - 1, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        for c in range(len(cptr) - 1):
            acc = np.float32(0)
            for v in cval[cptr[c]:cptr[c + 1]]:
                acc = np.float32(acc + np.float32(v * v))
            out[c] = acc
    return out


@functools.lru_cache(maxsize=None)
def sqnorm_case() -> Tuple[np.ndarray, np.ndarray]:
    """(cptr int32 [n + 1], cval float32): the head lengths around the 64-entry chunk, then columns of 0 .. 3 entries.
    Values: ordinary ones, 1e-20 (its square is a denormal), 1e-23 (its square underflows to 0), 1e19 in one column."""
    rng = np.random.default_rng(19)
    lens = np.concatenate([np.array(SQN_HEAD_LENGTHS), rng.integers(0, 4, SQN_N_ITEMS - len(SQN_HEAD_LENGTHS))])
    cptr = np.zeros(SQN_N_ITEMS + 1, dtype=np.int32)
    np.cumsum(lens, out=cptr[1:])
    n = int(cptr[-1])
    kind = rng.random(n)
    val = (rng.random(n) * 4.9 + 0.1) * np.where(rng.random(n) < 0.3, -1.0, 1.0)
    val = np.where(kind < 0.15, 1e-20, np.where(kind < 0.30, 1e-23, val)).astype(np.float32)
    b = int(cptr[SQN_INF_COLUMN])
    val[b + 100:b + 110] = np.float32(1e19)
    return cptr, val


@functools.lru_cache(maxsize=None)
def gram_exact_matrix(n_users: int, n_items: int = 400) -> sp.csc_matrix:
    """n_users x n_items, a tenth filled (at least one entry), ratings multiples of 0.5 in [0.5, 5]: every product is a multiple
    of 0.25 and every sum far below 2^53, so a float64 accumulation is exact in any order."""
    rng = np.random.default_rng(1000 + n_users)
    n = max(1, n_users * n_items // 10)
    u, i = rng.integers(0, n_users, n), rng.integers(0, n_items, n)
    key = np.unique(u * n_items + i)
    v = (rng.integers(1, 11, len(key)) * 0.5).astype(np.float32)
    X = sp.csc_matrix((v, (key // n_items, key % n_items)), shape=(n_users, n_items), dtype=np.float32)
    X.sort_indices()
    return X


def gram_top_items(n_items: int, n_top: int, seed: int, repeat: bool = False) -> np.ndarray:
    """n_top items in a seeded random order (neither sorted nor by popularity); repeat: the last one repeats the first."""
    top = np.random.default_rng(seed).permutation(n_items)[:n_top].astype(np.int32)
    if repeat and n_top > 1:
        top[-1] = top[0]
    return top


def gram_fsum(XP: np.ndarray) -> np.ndarray:
    """XP^T XP with every entry the exactly rounded sum (math.fsum) of its exact float64 products."""
    XP = np.asarray(XP, dtype=np.float64)
    P = XP.shape[1]
    ref = np.zeros((P, P), dtype=np.float64)
    for a in range(P):
        ua = np.flatnonzero(XP[:, a])
        for b in range(a, P):
            ref[a, b] = ref[b, a] = math.fsum((XP[ua, a] * XP[ua, b]).tolist())
    return ref


def gram_gamma(n: int) -> float:
    """The header's promise for non-negative data: |G - ref| <= g * ref with g = n 2^-53 / (1 - n 2^-53), n = n_users."""
    u = n * 2.0 ** -53
    return u / (1.0 - u)


# ------------------------------------------------------------------------------------------------ D: segment layout
@dataclass
class SegCase:
    n_items: int
    rows: np.ndarray            # int64, the COO of W sorted by (column, row)
    cols: np.ndarray
    vals: np.ndarray            # float32
    lo: int
    hi: int
    labels: np.ndarray          # int64 [n_items]
    T: int                      # the tile width the case is built for
    expect: Dict[Tuple[int, int], Tuple[int, bool]]     # (row item, tile) -> (entries, stored dense) of the segments the case names
    bounds: Dict[Tuple[int, int], int]                  # (row item, tile) -> bf16 bound word of the segments the case names

    def csc(self) -> sp.csc_matrix:
        W = sp.csc_matrix((self.vals, (self.rows, self.cols)), shape=(self.n_items, self.n_items), dtype=np.float32)
        W.sort_indices()
        assert W.nnz == len(self.vals)          # stored zeros stay stored
        return W


class _Cells:
    """(row, column) -> weight, written down cell by cell."""

    def __init__(self, n_items: int):
        self.n_items, self.d = n_items, {}

    @staticmethod
    def value(row: int, col: int) -> np.float32:
        v = 0.25 + ((row * 31 + col * 17) % 97) / 64.0
        return np.float32(-v if (row + col) % 3 == 0 else v)

    def put(self, row: int, col: int, val=None) -> None:
        assert (row, col) not in self.d and 0 <= row < self.n_items and 0 <= col < self.n_items
        self.d[(row, col)] = self.value(row, col) if val is None else np.float32(val)

    def run(self, row: int, col0: int, n: int) -> None:
        for c in range(col0, col0 + n):
            self.put(row, c)

    def case(self, lo: int, hi: int, T: int, labels=None, expect=None, bounds=None) -> SegCase:
        keys = sorted(self.d, key=lambda rc: (rc[1], rc[0]))
        r = np.array([k[0] for k in keys], dtype=np.int64)
        c = np.array([k[1] for k in keys], dtype=np.int64)
        v = np.array([self.d[k] for k in keys], dtype=np.float32)
        labels = np.arange(self.n_items, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
        return SegCase(self.n_items, r, c, v, lo, hi, labels, T, expect or {}, bounds or {})


SEG_LENGTHS = (1, 2, 63, 64, 65, 66, 255, 256)


def _f32_from_bits(b: int) -> np.float32:
    return np.array([b], dtype=np.uint32).view(np.float32)[0]


@functools.lru_cache(maxsize=None)
def seg_case(name: str) -> SegCase:
    """The constructed shards of part D.  Unless a case says otherwise labels = arange and a `spine` row holds a weight in
    every column of the layout, so layout column = item id - first column and a segment's length is what the case wrote."""
    if name == "lengths":
        # T = 256, 1023 columns (the last tile is 255 wide).  Middle tile 1: one row per length; last tile 3: one row per
        # length that fits, right-aligned, so each of them has an entry in the very last column.
        I = 1023
        w, expect = _Cells(I), {}
        w.run(1000, 0, I)
        for k, n in enumerate(SEG_LENGTHS):
            w.run(10 + k, 256 + (k * 37) % (256 - n + 1), n)
            expect[(10 + k, 1)] = (n, n > 64)
            if n <= 255:
                w.run(40 + k, I - n, n)
                expect[(40 + k, 3)] = (n, n > 64)
        w.run(70, 0, 64)                      # ... and the very first column
        expect[(70, 0)] = (64, False)
        expect[(1000, 3)] = (255, True)
        return w.case(0, I, 256, expect=expect)
    if name in ("cols_32768", "cols_32769"):
        # 32,768 active columns are 128 tiles of 256; one more and the tiles are 512 wide, where nothing is stored dense
        n_cols = int(name[5:])
        I = 33000
        w = _Cells(I)
        w.run(32999, 0, n_cols)
        w.run(5, 1280, 65)
        w.run(6, 2560, 64)
        w.put(7, n_cols - 1)
        if n_cols == 32768:
            return w.case(0, I, 256, expect={(5, 5): (65, True), (6, 10): (64, False), (7, 127): (1, False), (32999, 127): (256, True)})
        return w.case(0, I, 512, expect={(5, 2): (65, False), (6, 5): (64, False), (7, 64): (1, False), (32999, 0): (512, False)})
    if name == "one_column":
        w = _Cells(300)
        for r in (3, 150, 299):
            w.put(r, 77)
        return w.case(0, 300, 256, expect={(3, 0): (1, False), (299, 0): (1, False)})
    if name == "one_entry":
        w = _Cells(50)
        w.put(7, 9)
        return w.case(0, 50, 256, expect={(7, 0): (1, False)})
    if name == "shard_gaps":
        # columns [100, 500) of 600: most of them empty; rows 40 and 41 have entries only outside the shard
        w = _Cells(600)
        for c in (100, 101, 105, 250, 499):
            w.put(30, c)
        w.run(20, 300, 70)
        w.put(550, 499)
        w.put(550, 100)
        for c in (50, 550):
            w.put(40, c)
            w.put(41, c)
        w.put(20, 10)
        w.put(30, 599)
        return w.case(100, 500, 256, expect={(20, 0): (70, True), (30, 0): (5, False), (550, 0): (2, False)})
    if name == "key_end_pow2":
        # 4 rows x 2 tiles x 256 = 2^11: the key of the entries outside the shard is exactly 2^11
        w = _Cells(1000)
        w.run(5, 200, 300)
        for r, c in ((6, 200), (6, 499), (7, 455), (7, 456), (8, 300)):
            w.put(r, c)
        w.run(5, 0, 50)
        w.put(900, 800)
        w.put(6, 999)
        w.put(950, 199)
        w.put(951, 700)
        return w.case(200, 700, 256, expect={(5, 0): (256, True), (5, 1): (44, False), (7, 0): (1, False), (7, 1): (1, False)})
    if name.startswith("labels_"):
        # 4,096 items (a power of two: the sentinel label 4096 of the columns that hold nothing needs a thirteenth bit)
        I = 4096
        w = _Cells(I)
        for c in range(I):
            if c % 50 != 7:
                w.put(4000, c)
        for r, c in ((2, 1), (2, 2), (2, 3), (3, 4095), (3, 4094), (9, 0), (9, 2048)):
            w.put(r, c)
        w.run(12, 100, 90)
        ar = np.arange(I, dtype=np.int64)
        labels = {"labels_zero": np.zeros(I, dtype=np.int64), "labels_reversed": I - 1 - ar,
                  "labels_top_on_lowest": np.where(ar < 10, I - 1, ar)}[name]
        return w.case(0, I, 256, labels=labels)
    if name == "values":
        # -0.0, a denormal, FLT_MAX; a weight whose low 16 bits are zero (its bfloat16 bound is the weight) next to one
        # whose low bits are 0x0001 (the bound is one bfloat16 step up)
        I = 600
        w = _Cells(I)
        w.run(590, 0, I)
        flt_max, tiny = np.finfo(np.float32).max, np.float32(1e-40)
        lo16, lo16p = _f32_from_bits(0x3FC00000), _f32_from_bits(0x3FC00001)
        w.put(10, 5, -0.0)
        w.put(10, 300, tiny)
        w.put(10, 520, flt_max)
        w.put(10, 521, -1.0)
        w.put(11, 7, lo16)
        w.put(11, 8, 1.25)
        w.put(11, 260, lo16p)
        w.put(11, 261, lo16)
        w.put(11, 530, -lo16p)
        w.run(12, 20, 70)
        w.d[(12, 25)] = np.float32(-0.0)
        w.d[(12, 26)] = -tiny
        return w.case(0, I, 256, expect={(12, 0): (70, True), (10, 0): (1, False)},
                      bounds={(10, 0): 0, (10, 1): 2, (10, 2): 0x7F80, (11, 0): 0x3FC0, (11, 1): 0x3FC1, (11, 2): 0x3FC1})
    raise KeyError(name)


SEG_CASES = ("lengths", "cols_32768", "cols_32769", "one_column", "one_entry", "shard_gaps", "key_end_pow2", "labels_zero",
             "labels_reversed", "labels_top_on_lowest", "values")


def decode_seg_layout(L: Dict[str, Any], case: SegCase) -> Dict[str, Any]:
    """Reads a segment layout back (include/rtrec_amd.h, csrc/score_seg.hip.h) and holds it to the shard it was built from:
    the COO of W[:, lo:hi] rebuilt from sg_info / sg_ptr / sg_ent / sg_col_ids equals the input bit for bit, sg_bound is the
    bfloat16-rounded-up max |w| per (row, tile), sg_trow / sg_trow_ptr list exactly the non-empty segments per tile in
    ascending item order.  Asserts; returns what it found: T, n_tiles, n_rec, n_list, segments {(row item, tile): (n, dense)}
    and bound words {(row item, tile): uint16}.  Arrays may be longer than what is in use (the native builder allocates for
    the worst case).  A stored +0.0 inside a dense block cannot be told from an absent weight: the cases store none."""
    g = lambda k: np.asarray(L[k])
    T, n_tiles, R, n_cols = int(L["sg_T"]), int(L["sg_n_tiles"]), int(L["sg_rows"]), int(L["sg_n_cols"])
    I = case.n_items
    sel = (case.cols >= case.lo) & (case.cols < case.hi)
    r_in, c_in, b_in = case.rows[sel], case.cols[sel], f32_bits(case.vals[sel])
    labels = case.labels

    # columns: the active ones by (label, item); tiles of the smallest power of two >= 256 that needs at most 128 of them
    col_order = sorted(set(c_in.tolist()), key=lambda c: (int(labels[c]), c))
    assert n_cols == len(col_order)
    want_T = 256
    while -(-n_cols // want_T) > 128:
        want_T *= 2
    assert T == want_T and n_tiles == -(-n_cols // T)
    col_ids = g("sg_col_ids").astype(np.int64)
    assert col_ids.shape == (n_cols,) and col_ids.tolist() == col_order
    info = g("sg_info").astype(np.int64).reshape(I, 2)
    want_pos = np.full(I, -1, dtype=np.int64)
    want_pos[col_ids] = np.arange(n_cols)
    assert np.array_equal(info[:, 1], want_pos)
    row_items = sorted(set(r_in.tolist()))
    assert R == len(row_items)
    want_row = np.full(I, -1, dtype=np.int64)
    want_row[row_items] = np.arange(R)
    assert np.array_equal(info[:, 0], want_row)

    # records
    ptr = (g("sg_ptr").astype(np.int64) & 0xFFFFFFFF).reshape(R, n_tiles + 1)
    ent = np.ascontiguousarray(g("sg_ent")).astype(np.int32).reshape(-1, 2)
    out_r, out_c, out_b, segs, nxt = [], [], [], {}, 0
    for r in range(R):
        for t in range(n_tiles):
            dense, b, e = bool(ptr[r, t] >> 31), int(ptr[r, t] & 0x7FFFFFFF), int(ptr[r, t + 1] & 0x7FFFFFFF)
            assert b == nxt and e >= b and e <= ent.shape[0], (r, t)
            if dense:
                assert T == 256 and e - b == 128, (r, t)
                words = ent[b:e].reshape(-1)
                col_in = np.flatnonzero(words)
                wbits = words[col_in]
                n = len(col_in)
                assert n > 64, (r, t)
            else:
                rec = ent[b:e]
                n = e - b
                if n and rec[-1, 0] == T:                 # the {T, +0.0} pad
                    assert rec[-1, 1] == 0, (r, t)
                    n -= 1
                assert n + (n & 1) == e - b, (r, t)
                col_in, wbits = rec[:n, 0].astype(np.int64), rec[:n, 1]
                assert np.all((col_in >= 0) & (col_in < T)) and np.all(np.diff(col_in) > 0), (r, t)
                assert T > 256 or n <= 64, (r, t)
            assert np.all(t * T + col_in < n_cols), (r, t)
            out_r.extend([row_items[r]] * n)
            out_c.extend(col_ids[t * T + col_in].tolist())
            out_b.extend(wbits.view(np.uint32).tolist())
            segs[(row_items[r], t)] = (n, dense)
            nxt = e
        assert ptr[r, n_tiles] == nxt, r                   # a row's end pointer carries no flag
    n_rec = nxt
    got = sorted(zip(out_c, out_r, out_b))
    assert [x[0] for x in got] == c_in.tolist() and [x[1] for x in got] == r_in.tolist(), "rebuilt cells differ"
    assert [x[2] for x in got] == b_in.tolist(), "rebuilt weight bits differ"

    # bounds: bfloat16 of max |w|, rounded up, two tiles per word
    mx = {}
    lay = want_pos[c_in]
    for rr, pc, bb in zip(r_in.tolist(), lay.tolist(), b_in.tolist()):
        k = (rr, pc // T)
        mx[k] = max(mx.get(k, 0), bb & 0x7FFFFFFF)
    want_b = np.zeros((R, 64), dtype=np.uint32)
    words = {}
    for (rr, t), m in mx.items():
        up = (m >> 16) + (1 if m & 0xFFFF else 0)
        words[(rr, t)] = up
        want_b[want_row[rr], t // 2] |= np.uint32(up << (16 * (t & 1)))
    assert np.array_equal(np.ascontiguousarray(g("sg_bound")).view(np.uint32).reshape(R, 64), want_b), "sg_bound"
    assert set(mx) == {k for k, (n, _) in segs.items() if n > 0}

    # the tile-side lists
    tp = g("sg_trow_ptr").astype(np.int64)
    trow = g("sg_trow").astype(np.int64).reshape(-1, 4)
    assert tp.shape == (n_tiles + 1,) and tp[0] == 0
    at = 0
    for t in range(n_tiles):
        want = [[row_items[r], int(np.int64(ptr[r, t]).astype(np.int32)), int(ptr[r, t + 1] & 0x7FFFFFFF), 0]
                for r in range(R) if segs[(row_items[r], t)][0] > 0]
        assert tp[t] == at and tp[t + 1] == at + len(want), t
        assert trow[at:at + len(want)].tolist() == want, t
        at += len(want)
    return dict(T=T, n_tiles=n_tiles, n_rec=n_rec, n_list=at, segments=segs, bounds=words)
