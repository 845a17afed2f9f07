"""decay_kernel (csrc/store_device.hip) and HipBackend.decay_f32 on the GPU against libm, on inputs built to sit on float32
rounding boundaries (tests/test_decay_host.py: the builders, the numpy statement of the flag rule and the guards that the
inputs decide something).

The bit-exactness of a resident store with time decay rests on one statement: every entry whose device float32 differs from
libm's is among the entries the kernel lists.  Tests 1 and 2 pin the rule and that statement at the kernel, test 3 the patched
result, test 4 the list's capacity and the host-does-them-all branch, test 5 the rule's share on random data, test 6 a store
whose history reaches float32 denormals end to end."""
import numpy as np
import pytest

from tests.test_decay_host import (DECAY_DAYS, NOW, adversarial_sets, bits32, boundary_distance_ulps, boundary_set, concat_sets,
                                   flag_regimes, flag_rule, libm_decay, rate_of, store_decay, to_f32, LADDER_IN)

pytestmark = pytest.mark.gpu

POISON_F, POISON_I = 1234.5, -7


def run_kernel(val, ts, rate, now=NOW, cap=None, slack=64):
    """One store_decay_device call on poisoned outputs: (out float32[n], listed indices int[min(count, cap)], count, the
    words of the index buffer beyond cap)."""
    import torch
    n = len(val)
    cap = n if cap is None else cap
    dev = "cuda:0"
    out = torch.full((n,), POISON_F, dtype=torch.float32, device=dev)
    buf = torch.full((cap + slack,), POISON_I, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), 99, dtype=torch.int32, device=dev)
    torch.ops.rtrec_amd.store_decay_device(torch.from_numpy(np.ascontiguousarray(val, dtype=np.float64)).to(dev),
                                           torch.from_numpy(np.ascontiguousarray(ts, dtype=np.float64)).to(dev),
                                           float(rate), float(now), out, buf[:cap], cnt)
    torch.cuda.synchronize()
    k, buf = int(cnt.item()), buf.cpu().numpy()
    return out.cpu().numpy(), buf[:min(k, cap)], k, buf[cap:]


def same_f32(a, b):
    """Bit for bit, the sign of zero included; NaN compared by isnan."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits32(a)[~na], bits32(b)[~nb])


def backend():
    import rtrec_amd  # noqa: F401  (registers the ops)
    from rtrec_amd.backend import HipBackend
    return HipBackend("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _ops():
    backend()


# ---------------------------------------------------------------------------------------------- 1: the rule, exactly
def test_flag_set_equals_the_rule_when_pow_is_one():
    """ts == now: pow(rate, 0) is exactly 1, the device product is val itself -- so the listed set must EQUAL flag_rule(val) and
    out must be float32(val), in every regime of the rule (normals, powers of two, FLT_MIN, denormals, both signs, +-0.0,
    NaN, inf, 1e300 and more, the underflow and the overflow zone, the margin's own edge)."""
    val = flag_regimes()
    ts = np.full(val.shape[0], NOW)
    for days in (7, 3650):
        out, idx, k, beyond = run_kernel(val, ts, rate_of(days))
        assert same_f32(out, to_f32(val))
        want = np.flatnonzero(flag_rule(val))
        assert k == len(idx) == len(set(idx.tolist())), "an entry is listed once"
        got = np.sort(idx)
        missing, extra = np.setdiff1d(want, got), np.setdiff1d(got, want)
        assert missing.size == 0 and extra.size == 0, (f"rule flags {len(want)}, kernel {k}; not listed: {val[missing][:6]!r}, "
                                                       f"listed against the rule: {val[extra][:6]!r}")
        assert (beyond == POISON_I).all()
        assert 0.05 * len(val) < k < 0.6 * len(val)


# ---------------------------------------------------------------------------------------------- 2: the invariant
def test_entries_that_differ_from_libm_are_flagged_and_must_flag_entries_all_are():
    """Real elapsed times, the device's own pow: {device float32 != libm float32} is a subset of the listed entries, and
    every inside-ladder, underflow and overflow entry is listed.  Prints what was measured: how many entries the device and
    libm disagree on before patching, and how far from a boundary (in 2^-52 |v|) the farthest of them lies -- the headroom
    under the margin of 4096."""
    n_diff = n_all = 0
    worst = 0.0
    for s in adversarial_sets():
        out, idx, k, _ = run_kernel(s.val, s.ts, s.rate)
        v, f = libm_decay(s.val, s.ts, s.rate)
        listed = np.zeros(len(v), bool)
        listed[idx] = True
        assert k == len(idx) == int(listed.sum())
        differs = ~((bits32(out) == bits32(f)) | (np.isnan(out) & np.isnan(f)))
        stray = differs & ~listed
        assert not stray.any(), (s.name, int(stray.sum()), s.val[stray][:4], s.ts[stray][:4], out[stray][:4], f[stray][:4])
        if s.must_flag:
            assert listed.all(), (s.name, int((~listed).sum()), s.val[~listed][:4], s.step[~listed][:4])
        if s.kind == "skip":
            assert not listed.any() and not differs.any(), s.name
        if s.kind in ("inside", "outside"):
            d = boundary_distance_ulps(v)[differs]
            worst = max(worst, float(d.max()) if d.size else 0.0)
        n_diff, n_all = n_diff + int(differs.sum()), n_all + len(v)
        print(f"{s.name}: {len(v)} entries, {k} listed, {int(differs.sum())} differ from libm before patching")
    print(f"adversarial sets: device and libm float32 differ on {n_diff} of {n_all} entries before patching; the farthest of them "
          f"lies {worst:.1f} x 2^-52 |v| from its boundary (margin: 4096)")


# ---------------------------------------------------------------------------------------------- 3: the patched result
@pytest.mark.parametrize("days", DECAY_DAYS)
def test_decay_f32_equals_libm_on_the_adversarial_sets(days):
    import torch
    be = backend()
    sets = [s for s in adversarial_sets() if s.days == days]
    val, ts, _ = concat_sets(sets)
    got = be.decay_f32(torch.from_numpy(val).to(be.device), torch.from_numpy(ts).to(be.device), sets[0].rate, NOW).cpu().numpy()
    _, want = libm_decay(val, ts, sets[0].rate)
    assert got.dtype == np.float32 and same_f32(got, want), np.flatnonzero(bits32(got) != bits32(want))[:8]
    assert (want == 0).any() and np.signbit(want[want == 0]).any() and np.isinf(want).any() and np.isnan(want).any()


# ---------------------------------------------------------------------------------------------- 4: the cap
def test_list_capacity_is_respected_and_decay_f32_hands_everything_to_the_host_beyond_it():
    import torch
    hard = boundary_set(30, LADDER_IN, "inside", seed=901, n_base=160)  # 4000 entries, each one must be listed
    assert len(hard.val) == 4000 and flag_rule(libm_decay(hard.val, hard.ts, hard.rate)[0]).all()
    out, idx, k, beyond = run_kernel(hard.val[:100], hard.ts[:100], hard.rate, cap=8, slack=120)
    assert k == 100, "the count is the true number of flagged entries, not the capacity"
    assert len(idx) == 8 and len(set(idx.tolist())) == 8 and ((idx >= 0) & (idx < 100)).all()
    assert (beyond == POISON_I).all(), "written past the list's capacity"
    assert (out != POISON_F).all()
    # decay_f32 beyond its capacity max(1024, n >> 10): "let the host do them all"
    n = 1_200_000
    rng = np.random.default_rng(41)
    val = rng.random(n) * 15.0 + 1e-3
    ts = NOW - rng.random(n) * 400 * 86400.0
    at = rng.choice(n, len(hard.val), replace=False)
    val[at], ts[at] = hard.val, hard.ts
    assert len(hard.val) > max(1024, n >> 10)                           # 4000 must-flag entries, capacity 1171
    be = backend()
    d_val, d_ts = torch.from_numpy(val).to(be.device), torch.from_numpy(ts).to(be.device)
    _, _, k, _ = run_kernel(val, ts, hard.rate, cap=max(1024, n >> 10))
    assert k > max(1024, n >> 10), k
    got = be.decay_f32(d_val, d_ts, hard.rate, NOW).cpu().numpy()
    _, want = store_decay(val, ts, hard.rate)
    assert same_f32(got, want)
    assert same_f32(want[at], libm_decay(hard.val, hard.ts, hard.rate)[1])


# ---------------------------------------------------------------------------------------------- 5: random data
def test_random_sweep_invariant_and_flagged_share():
    """4 M random entries (values in (0, 15], up to 400 days of history, 30-day decay): the invariant of test 2, and a listed
    share above 0 and at most 2^-14 -- the rule's geometry puts it between 2^-16 and 2^-15 (tests/test_decay_host.py), the
    factor of two covers the sampling noise on ~100 expected hits."""
    rng = np.random.default_rng(2024)
    n = 1 << 22
    val = 15.0 * (1.0 - rng.random(n))
    ts = NOW - rng.random(n) * 400 * 86400.0
    rate = rate_of(30)
    out, idx, k, _ = run_kernel(val, ts, rate, cap=1 << 16)
    v, f = store_decay(val, ts, rate)
    listed = np.zeros(n, bool)
    listed[idx] = True
    differs = bits32(out) != bits32(f)
    print(f"random sweep: {n} entries, {k} listed (share {k / n:.3e} = 2^{np.log2(max(k, 1) / n):.2f}), {int(differs.sum())} differ "
          f"from libm before patching; the rule on libm's products lists {int(flag_rule(v).sum())}")
    assert k == len(idx) and not (differs & ~listed).any()
    assert 0 < k <= n * 2.0 ** -14, (k, n)


# ---------------------------------------------------------------------------------------------- 6: end to end
def test_five_years_of_weekly_decay_through_the_resident_store_equals_host_exports(monkeypatch):
    """SLIM(min_value=-5, max_value=10, decay_in_days=7) over five years of timestamps with some negative ratings: a 1.0 is a
    float32 denormal after ~2.7 years and +-0.0 after ~2.9, so every old entry is in the kernel's underflow zone and
    decay_f32 takes its host-does-them-all branch.  bulk_fit and fit mini-batches with the device-resident store and with
    host exports: the resident X equals interactions.to_csr(), W and the recommendations are the same, bit for bit."""
    import scipy.sparse as sp
    from rtrec_amd import SLIM
    from tests.test_gpu_api import same_matrix
    rng = np.random.default_rng(19)
    U, I, n = 1200, 250, 30_000
    u, i = rng.integers(0, U, n), rng.zipf(1.3, n) % I
    r = (rng.integers(1, 6, n) * np.exp(-rng.random(n))).astype(float) * np.where(rng.random(n) < 0.15, -1.0, 1.0)
    # every other interaction falls in the last three weeks: with a 7-day half-life only those carry weight, and uniform
    # timestamps leave too little of it for the elastic net's l1 term (0.01 * U) to let any weight of W be non-zero
    span = 5 * 365 * 86400.0
    ts = 1.6e9 + np.sort(np.where(np.arange(n) % 2 == 0, rng.random(n) * span, span - rng.random(n) * 21 * 86400.0))
    n_bulk = n - 4 * 300

    def run(device_store):
        monkeypatch.setenv("RTREC_AMD_DEVICE_STORE", "1" if device_store else "0")
        m = SLIM(min_value=-5, max_value=10, decay_in_days=7, nn_feature_selection=8)
        m.add_interactions(list(zip(u[:n_bulk].tolist(), i[:n_bulk].tolist(), ts[:n_bulk].tolist(), r[:n_bulk].tolist())))
        m.bulk_fit(parallel=True, progress_bar=False)
        assert (m._dev_x is not None and m._dev_x.version == m._store_tag()) == device_store
        out = []
        for k in range(4):
            a = n_bulk + 300 * k
            m.fit(list(zip((u[a:a + 300] + (20 * k if k % 2 else 0)).tolist(), i[a:a + 300].tolist(), ts[a:a + 300].tolist(),
                           r[a:a + 300].tolist())), progress_bar=False)
            X = m.interactions.to_csr()
            X.sort_indices()
            if device_store:
                assert m._dev_x.version == m._store_tag() and m._dev_x.nnz == m.interactions.nnz
                F = m._dev_x.full()
                R = sp.csr_matrix((F["rval"].cpu().numpy(), F["rcol"].cpu().numpy(), F["rptr"].cpu().numpy()), shape=X.shape)
                assert same_matrix(R, X), "the resident X is not the host export"
            out.append((X.copy(), m.model.item_similarity.copy(), m.recommend_batch(list(range(0, 300, 3)), top_k=7)))
        return out

    dev, host = run(True), run(False)
    for (Xd, Wd, rd), (Xh, Wh, rh) in zip(dev, host):
        assert same_matrix(Xd, Xh) and same_matrix(Wd, Wh) and rd == rh
    d = dev[-1][0].data
    tiny = np.abs(d[d != 0]).min()
    assert tiny < 1.1754944e-38, "no float32 denormal among the stored values"
    assert (d == 0).any() and np.signbit(d[d == 0]).any() and (~np.signbit(d[d == 0])).any() and (d < 0).any()
    assert dev[-1][1].nnz > 100 and any(rd for rd in dev[-1][2])
