"""Time decay of a resident store (decay_kernel in csrc/store_device.hip, HipBackend.decay_f32) without a GPU: the kernel's flag
rule as numpy, the adversarial input builders, and the guards that show those inputs decide something.  The kernel itself is
in tests/test_gpu_decay.py, which imports the rule and the builders from here.

The scheme under test: the device computes float32(raw * pow(rate, (now - ts) / 86400)) with its own pow (not libm's bit for
bit), flags every entry whose float64 product lies within kMarginUlps = 4096 float64 ulps of a float32 rounding boundary -- or
where the float32 has no finite non-zero neighbour on both sides: the underflow and the overflow zone -- and the host patches
exactly those with libm.  "Every other float32 is the reference's" holds only if the rule is right and the device pow's error
stays below the margin; random data lands within an ulp or two of a boundary about once in 10^8 entries, so the sets here are
BUILT to sit on the boundaries: val = midpoint / pow(rate, elapsed), stepped by a ladder of float64 ulps.

Reference: math.pow per scalar (CPython's libm call, what the reference's `**` evaluates) -- never np.power, whose vectorised
float64 path need not equal libm.  rtrec_store_decay is asserted equal to it on every set, bits of float64 and of float32."""
import functools
import math
from dataclasses import dataclass

import numpy as np
import pytest

MARGIN_ULPS = 4096.0                       # kMarginUlps of csrc/store_device.hip
FLT_MAX = np.float32(3.4028234663852886e38)
FLT_MIN_BITS = 0x00800000                  # smallest normal float32
OVERFLOW_EDGE = 2.0 ** 128 - 2.0 ** 103    # float32 rounds to FLT_MAX below it, to inf from it on
NOW = 1.75e9
DECAY_DAYS = (1, 7, 30, 180, 3650)
LADDER_IN = tuple(2 ** j for j in range(12))           # relative distance d * 2^-52 (half of it at worst): inside the margin
LADDER_OUT = (2 ** 15, 2 ** 17, 2 ** 20, 2 ** 24)      # at least 2^14 * 2^-52 whatever the binade of val: outside
P_STEPS = (-2, -1, 0, 1, 2)                            # ulps of pow's result: the stand-in for a foreign pow


def rate_of(days: int) -> float:
    from rtrec_amd.utils.interactions import UserItemInteractions
    return float(UserItemInteractions(decay_in_days=days).decay_rate)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def to_f32(v):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(np.float32)


def step_ulps(x, d):
    """x moved by d float64 ulps away from zero (d < 0: towards it); x finite, non-zero and normal."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    mag = (np.abs(x).view(np.int64) + np.asarray(d, np.int64)).view(np.float64)
    return np.copysign(mag, x)


# ---------------------------------------------------------------------------------------------- the kernel's rule
def flag_rule(v):
    """decay_kernel's decision for the float64 product v, statement by statement (bool array: the entry is listed)."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = v.astype(np.float32)
        a, af = np.abs(v), np.abs(f)
        decides = (a < 1e300) & (v != 0.0)                       # inf / NaN / |v| >= 1e300 / an exact zero: nothing to decide
        # no finite non-zero neighbour on both sides: underflow (rounds to 0, or below 2^-148) and overflow (FLT_MAX or inf)
        edge = (f == 0) | (a < 2.0 ** -148) | ~(af < FLT_MAX)
        b = af.view(np.uint32)
        fd = af.astype(np.float64)
        up = (b + np.uint32(1)).view(np.float32).astype(np.float64)
        dn = (b - np.uint32(1)).view(np.float32).astype(np.float64)
        m_up, m_dn = 0.5 * (fd + up), 0.5 * (fd + dn)
        dist = np.fmin(np.abs(a - m_up), np.abs(a - m_dn))
        near = dist <= MARGIN_ULPS * 2.0 ** -52 * a
    return decides & (edge | near)


def boundary_distance_ulps(v):
    """Distance of v to the nearest float32 rounding boundary in units of 2^-52 |v| (inf where there is none to measure:
    zeros, non-finite products, the overflow zone) -- a measurement, not part of the rule."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = v.astype(np.float32)
        a, af = np.abs(v), np.abs(f)
        b = af.view(np.uint32)
        fd = af.astype(np.float64)
        up = (b + np.uint32(1)).view(np.float32).astype(np.float64)
        dn = np.where(b > 0, (b - np.uint32(1)).view(np.float32).astype(np.float64), -fd)
        up = np.where(af < FLT_MAX, up, 2.0 ** 128)
        dist = np.fmin(np.abs(a - 0.5 * (fd + up)), np.abs(a - 0.5 * (fd + dn)))
        out = dist / (2.0 ** -52 * a)
    return np.where(np.isfinite(v) & (v != 0) & np.isfinite(out), out, np.inf)


# ---------------------------------------------------------------------------------------------- reference
def libm_pow(rate: float, ts, now: float = NOW):
    return np.array([math.pow(rate, (now - float(t)) / 86400.0) for t in np.asarray(ts, np.float64)], np.float64)


def libm_decay(val, ts, rate: float, now: float = NOW):
    """(float64 products, float32 casts): val * math.pow(rate, (now - ts) / 86400.0), one Python float expression per entry."""
    val = np.asarray(val, np.float64)
    with np.errstate(all="ignore"):
        v = np.array([float(x) * math.pow(rate, (now - float(t)) / 86400.0) for x, t in zip(val, np.asarray(ts, np.float64))],
                     np.float64)
    return v, to_f32(v)


def store_decay(val, ts, rate: float, now: float = NOW):
    """The same through rtrec_store_decay (the host routine the kernel's flagged entries are patched with)."""
    from rtrec_amd import _native
    L = _native.load()
    val, ts = np.ascontiguousarray(val, dtype=np.float64), np.ascontiguousarray(ts, dtype=np.float64)
    o64, o32 = np.empty(val.shape[0], np.float64), np.empty(val.shape[0], np.float32)
    assert L.rtrec_store_decay(val.ctypes.data, ts.ctypes.data, val.shape[0], float(rate), None, float(now), o64.ctypes.data,
                               o32.ctypes.data, 0) == 0
    return o64, o32


# ---------------------------------------------------------------------------------------------- input builders
@dataclass
class DecaySet:
    name: str
    kind: str              # "inside" | "outside" | "underflow" | "overflow" | "skip": what the rule must do with every entry
    days: int
    rate: float
    val: np.ndarray        # raw stored values (float64)
    ts: np.ndarray         # their timestamps (float64); now = NOW
    step: np.ndarray       # the ladder step of each entry (int64; 0 where there is no ladder)
    now: float = NOW

    @property
    def must_flag(self) -> bool:
        return self.kind in ("inside", "underflow", "overflow")


def elapsed_timestamps(rng, rate: float, n: int, p_min: float = 2.0 ** -200):
    """n timestamps from `now` back to where pow(rate, elapsed) is about p_min (every fourth one is `now` itself or a whole
    number of days back), and libm's pow for each."""
    e_max = math.log(p_min) / math.log(rate)
    e = rng.random(n) * e_max * rng.random(n) ** 2          # denser near the present, reaching the far end
    e[::4] = np.floor(e[::4])
    e[::16] = 0.0
    e[1] = e_max
    ts = NOW - e * 86400.0
    return ts, libm_pow(rate, ts)


def boundary_floats(rng, n: int, denormal_from: int = 1):
    """n positive float32 numbers f (as uint32 bit patterns) whose upper neighbour g = f + 1 ulp is finite, a fifth from each
    regime: random normals; powers of two (f = 2^k: the midpoint above it); their predecessors (g = 2^k: the midpoint below
    a power of two, where the lower neighbour of g is half as far as the upper); FLT_MIN and the largest denormal; denormals
    with bit patterns from `denormal_from`."""
    k = n // 5
    expo = rng.integers(1, 254, k).astype(np.uint32)
    normal = (expo << np.uint32(23)) | rng.integers(0, 1 << 23, k).astype(np.uint32)
    pow2 = rng.integers(2, 254, k).astype(np.uint32) << np.uint32(23)
    below = (rng.integers(2, 254, k).astype(np.uint32) << np.uint32(23)) - np.uint32(1)
    edge = np.where(rng.random(k) < 0.5, FLT_MIN_BITS, FLT_MIN_BITS - 1).astype(np.uint32)
    den = np.concatenate([np.arange(denormal_from, denormal_from + 8), rng.integers(denormal_from, 1 << 23, n - 4 * k - 8)]).astype(np.uint32)
    return np.concatenate([normal, pow2, below, edge, den])


def boundary_set(days: int, ladder, kind: str, seed: int, n_base: int = 400) -> DecaySet:
    """Products ON float32 rounding boundaries: for a random elapsed time with p = math.pow(rate, e) and a float32 f with upper
    neighbour g, m = (f + g) / 2 is exact in float64; val = m / p makes val * p equal m to an ulp, and the ladder moves val by
    +-d float64 ulps (d = 0 included for the inside ladder).  Both signs of val."""
    rng = np.random.default_rng(seed)
    rate = rate_of(days)
    ts, p = elapsed_timestamps(rng, rate, n_base)
    fb = boundary_floats(rng, n_base, denormal_from=1 if kind == "inside" else 16)
    rng.shuffle(fb)
    f = fb.view(np.float32).astype(np.float64)
    g = (fb + np.uint32(1)).view(np.float32).astype(np.float64)
    m = 0.5 * (f + g)
    assert np.array_equal(m - f, g - m)                            # the midpoint is exact
    base = (m / p) * np.where(rng.random(n_base) < 0.5, -1.0, 1.0)
    steps = np.array(([0] if kind == "inside" else []) + [s * d for d in ladder for s in (1, -1)], np.int64)
    val = step_ulps(np.repeat(base, len(steps)), np.tile(steps, n_base))
    return DecaySet(f"{kind}_d{days}", kind, days, rate, val, np.repeat(ts, len(steps)), np.tile(steps, n_base))


def edge_set(days: int, kind: str, seed: int, n_base: int = 120) -> DecaySet:
    """underflow: products within a few ulps of 2^-150 (float32 rounds to 0 or to the smallest denormal) and of 1.5 * 2^-149
    (to the smallest or the second denormal), and far below (1e-300, 1e-60).  overflow: within a few ulps of 2^128 - 2^103
    (float32 rounds to FLT_MAX or to inf).  Both signs."""
    rng = np.random.default_rng(seed)
    rate = rate_of(days)
    ts, p = elapsed_timestamps(rng, rate, n_base)
    targets = (2.0 ** -150, 1.5 * 2.0 ** -149, 1e-300, 1e-60) if kind == "underflow" else (OVERFLOW_EDGE,)
    t = np.array(targets)[rng.integers(0, len(targets), n_base)]
    base = (t / p) * np.where(rng.random(n_base) < 0.5, -1.0, 1.0)
    steps = np.arange(-4, 5, dtype=np.int64)
    val = step_ulps(np.repeat(base, len(steps)), np.tile(steps, n_base))
    return DecaySet(f"{kind}_d{days}", kind, days, rate, val, np.repeat(ts, len(steps)), np.tile(steps, n_base))


def skip_set(days: int) -> DecaySet:
    """What the kernel never lists: products of 1e300 and more, inf, NaN, exact zeros of both signs (a recent timestamp, so
    that a huge value stays huge)."""
    val = np.array([1e305, -1e305, 1.5e300, np.inf, -np.inf, np.nan, 0.0, -0.0, 1.7e308])
    ts = np.full(val.shape[0], NOW - 3600.0)
    ts[::2] = NOW
    return DecaySet(f"skip_d{days}", "skip", days, rate_of(days), val, ts, np.zeros(val.shape[0], np.int64))


@functools.lru_cache(maxsize=None)
def adversarial_sets():
    """Every set, for every decay rate: inside ladder, outside ladder, underflow, overflow, skip."""
    out = []
    for n, days in enumerate(DECAY_DAYS):
        out += [boundary_set(days, LADDER_IN, "inside", 100 + n), boundary_set(days, LADDER_OUT, "outside", 200 + n),
                edge_set(days, "underflow", 300 + n), edge_set(days, "overflow", 400 + n), skip_set(days)]
    return tuple(out)


def concat_sets(sets):
    """(val, ts, must_flag) of several sets of ONE rate glued together."""
    assert len({s.rate for s in sets}) == 1
    return (np.concatenate([s.val for s in sets]), np.concatenate([s.ts for s in sets]),
            np.concatenate([np.full(s.val.shape[0], s.must_flag) for s in sets]))


def flag_regimes():
    """Products for a call with ts == now (pow is exactly 1, the device product is val itself): (val, label) covering every
    regime of the rule -- midpoints of normals, powers of two, FLT_MIN, denormals with the ladder around each and the
    margin's own edge (4095 / 4096 / 4097 ulps and the binade-dependent factor), random values far from any boundary, both
    signs, +-0.0, NaN, inf, 1e300 and more, the underflow and the overflow sets."""
    rng = np.random.default_rng(77)
    fb = boundary_floats(rng, 600)
    f = fb.view(np.float32).astype(np.float64)
    g = (fb + np.uint32(1)).view(np.float32).astype(np.float64)
    m = 0.5 * (f + g)
    steps = np.array([0] + [s * d for d in LADDER_IN + (4095, 4096, 4097, 6000, 8191, 8192, 8193) + LADDER_OUT for s in (1, -1)], np.int64)
    ladder = step_ulps(np.repeat(m, len(steps)), np.tile(steps, len(m)))
    exact = np.concatenate([f, g])                                           # float32 numbers themselves: half a spacing away
    rnd = rng.random(20_000) * 15.0 + 1e-3
    wide = np.exp(rng.uniform(np.log(1e-44), np.log(3e38), 20_000))          # log-uniform over float32's whole range
    under = np.concatenate([step_ulps(np.full(9, t), np.arange(-4, 5)) for t in (2.0 ** -150, 1.5 * 2.0 ** -149, 2.0 ** -148, 2.0 ** -149)]
                           + [np.array([1e-300, 1e-60, 5e-324, 2.0 ** -1022, 2.0 ** -151])])
    over = np.concatenate([step_ulps(np.full(17, OVERFLOW_EDGE), np.arange(-8, 9)), np.array([2.0 ** 128, 1e39, 1e299, 9.99e299]),
                           np.float64(FLT_MAX) + np.array([0.0, 2.0 ** 100, -2.0 ** 100, -2.0 ** 102, -2.0 ** 103])])
    pos = np.concatenate([ladder, exact, rnd, wide, under, over])
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e300, -1e300, 1.0000001e300, 1.7e308, -1.7e308])
    return np.concatenate([pos, -pos, special])


# ---------------------------------------------------------------------------------------------- the rule, by hand
def test_flag_rule_on_cases_worked_out_by_hand():
    one, nxt = 1.0, float(np.nextafter(np.float32(1), np.float32(2)))
    mid = 0.5 * (one + nxt)                                   # 1 + 2^-24
    below = 1.0 - 2.0 ** -25                                  # midpoint between 1 and its LOWER neighbour 1 - 2^-24
    case = lambda x: bool(flag_rule(np.array([x]))[0])
    assert case(mid) and case(-mid) and case(below)
    ulp = 2.0 ** -52                                          # of numbers in [1, 2)
    assert case(mid + 4096 * ulp) and case(mid - 4096 * ulp) and not case(mid + 4097 * ulp) and not case(mid - 4097 * ulp)
    assert case(below - 8191 * ulp / 2) and not case(below - 8193 * ulp / 2)      # below 1 a float64 ulp is 2^-53: the margin
                                                                                  # is relative to |v|, not a count of ulps
    assert not case(1.0) and not case(1.5) and not case(nxt) and not case(-3.25)
    # skip cases
    assert not any(flag_rule(np.array([np.inf, -np.inf, np.nan, 1e300, -1e300, 1.7e308, 0.0, -0.0])))
    assert case(9.99e299)                                     # finite, below 1e300, float32 inf: the overflow zone
    # underflow: everything that rounds to zero or lies below 2^-148, however far
    for x in (2.0 ** -150, 2.0 ** -150 * (1 + 2 ** -50), 2.0 ** -150 * (1 - 2 ** -50), 1.5 * 2.0 ** -149, 2.0 ** -149, 1e-300, 5e-324, -1e-60):
        assert case(x), x
    assert not case(2.0 ** -148) and case(2.5 * 2.0 ** -149) and not case(2.0 ** -140)     # 2.5 denormal spacings: a midpoint
    # overflow: FLT_MAX or inf as the float32 of a finite product
    for x in (OVERFLOW_EDGE, float(FLT_MAX), OVERFLOW_EDGE * (1 - 2.0 ** -52), 2.0 ** 128, 1e39, -OVERFLOW_EDGE, -float(FLT_MAX)):
        assert case(x), x
    below_max = float(np.nextafter(FLT_MAX, np.float32(0)))
    assert not case(below_max) and case(0.5 * (below_max + float(FLT_MAX)))
    assert to_f32(OVERFLOW_EDGE * (1 - 2.0 ** -52)) == FLT_MAX and np.isinf(to_f32(OVERFLOW_EDGE))


def test_flag_rule_share_of_random_entries_lies_between_2_pow_minus_16_and_minus_15():
    """Two boundaries per float32 spacing (2^-24 .. 2^-23 of |v|), a band of 2 * 4096 * 2^-52 |v| around each: a share of
    2^-16 .. 2^-15 of random products, depending on where in the binade they fall."""
    rng = np.random.default_rng(3)
    n = 2_000_000
    val = rng.random(n) * 15.0 + 1e-6
    ts = NOW - rng.random(n) * 400 * 86400.0
    v, _ = store_decay(val, ts, rate_of(30))
    share = flag_rule(v).mean()
    print(f"flag_rule on {n} random entries: share {share:.3e} (2^-16 = {2.0 ** -16:.3e}, 2^-15 = {2.0 ** -15:.3e})")
    assert 2.0 ** -17 <= share <= 2.0 ** -14, share       # 30 to 61 expected hits: a factor of two covers the sampling noise


# ---------------------------------------------------------------------------------------------- reference
def test_store_decay_is_math_pow_on_every_adversarial_set():
    n = 0
    for s in adversarial_sets():
        v, f = libm_decay(s.val, s.ts, s.rate)
        o64, o32 = store_decay(s.val, s.ts, s.rate)
        assert np.array_equal(bits64(o64)[~np.isnan(v)], bits64(v)[~np.isnan(v)]) and np.array_equal(np.isnan(o64), np.isnan(v)), s.name
        assert np.array_equal(bits32(o32)[~np.isnan(f)], bits32(f)[~np.isnan(f)]) and np.array_equal(np.isnan(o32), np.isnan(f)), s.name
        n += len(v)
    assert n > 70_000


# ---------------------------------------------------------------------------------------------- input guards
def _perturbed_products(s: DecaySet, d: int):
    """val * (math.pow's result moved by d ulps): what a foreign pow with that error would hand the rule."""
    p = libm_pow(s.rate, s.ts)
    with np.errstate(all="ignore"):
        return s.val * (step_ulps(p, d) if d else p)


@pytest.mark.parametrize("days", DECAY_DAYS)
def test_every_inside_underflow_and_overflow_entry_is_flagged_whatever_the_pow(days):
    for s in adversarial_sets():
        if s.days != days or not s.must_flag:
            continue
        for d in P_STEPS:
            fl = flag_rule(_perturbed_products(s, d))
            assert fl.all(), (s.name, d, int((~fl).sum()), s.val[~fl][:4], s.step[~fl][:4])


@pytest.mark.parametrize("days", DECAY_DAYS)
def test_no_outside_entry_is_flagged_and_no_skip_entry(days):
    for s in adversarial_sets():
        if s.days != days or s.must_flag:
            continue
        for d in P_STEPS:
            fl = flag_rule(_perturbed_products(s, d))
            assert not fl.any(), (s.name, d, int(fl.sum()), s.val[fl][:4], s.step[fl][:4])


def test_the_sets_cover_what_they_claim():
    """Elapsed times from zero to where the product has long underflowed in float32, both signs, every float32 regime, products
    that are float32 denormals, zeros of both signs, FLT_MAX and inf."""
    for s in adversarial_sets():
        v, f = libm_decay(s.val, s.ts, s.rate)
        p = libm_pow(s.rate, s.ts)
        assert s.kind == "skip" or ((s.ts == s.now).any() and p.min() < 1e-45 and (p == 1.0).any()), s.name
        if s.kind in ("inside", "outside"):
            assert (s.val > 0).any() and (s.val < 0).any()
            b = bits32(np.abs(f))
            assert (b < FLT_MIN_BITS).sum() > 100 and ((b & 0x7FFFFF) == 0).sum() > 100 and (b == FLT_MIN_BITS).any(), s.name
            assert np.isfinite(s.val).all() and np.abs(s.val).max() < 1e200
        if s.kind == "underflow":
            assert (f == 0).any() and np.signbit(f[f == 0]).any() and (~np.signbit(f[f == 0])).any()
            assert (bits32(np.abs(f)) == 1).any() and (bits32(np.abs(f)) == 2).any() and (np.abs(v) < 1e-290).any()
        if s.kind == "overflow":
            assert np.isinf(f).any() and (np.abs(f) == FLT_MAX).any() and (f < 0).any() and np.isfinite(v).all()
        if s.kind == "skip":
            assert (np.abs(v[np.isfinite(v)]) >= 1e300).sum() >= 3 and np.isnan(v).any() and np.isinf(v).any()
    v = flag_regimes()
    fl = flag_rule(v)
    assert 0.05 < fl.mean() < 0.6 and len(v) > 100_000, fl.mean()


def test_on_the_boundary_a_pow_one_ulp_off_changes_the_float32():
    """Without this the sets decide nothing: at ladder step 0 a share of the entries must round to ANOTHER float32 when pow's
    result moves by one ulp (measured when the sets were built: about 30 %)."""
    changed = total = 0
    for s in adversarial_sets():
        if s.kind != "inside":
            continue
        at0 = s.step == 0
        f0 = bits32(to_f32(_perturbed_products(s, 0)[at0]))
        moved = np.zeros(f0.shape[0], bool)
        for d in (-1, 1):
            moved |= bits32(to_f32(_perturbed_products(s, d)[at0])) != f0
        changed, total = changed + int(moved.sum()), total + len(moved)
    print(f"step 0: {changed} of {total} entries change their float32 under a pow one ulp off ({changed / total:.1%})")
    assert total >= 2000 and changed >= 0.15 * total, (changed, total)
