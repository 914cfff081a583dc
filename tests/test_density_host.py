"""CPU: the host half of density estimation (include/sar.h: sar_density_*) against the numpy restatement
(tests/density_restatement.py) — the weight tables row for row, what every row must satisfy, the radius, the refusals, the default —
and the restatement itself held to properties known independently of it: mass conservation in Q16, the symmetries of the lattice,
the identity case. No device needed."""
import numpy as np
import pytest

import density_cases as K
import density_restatement as D

ALL_S = pytest.mark.parametrize("S", K.SAMPLES)


def _lattice(S):
    R = D.radius(S)
    return [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]


# ---- the library's tables ------------------------------------------------------------------------------------------------------
@ALL_S
def test_weights_equal_the_plan(sar, S):
    plan = D.plan(S)
    for c in range(1, S + 1):
        got = sar.density_weights(S, c)
        assert got.dtype == np.uint32 and np.array_equal(got, plan[c]), f"S {S} class {c}: {got[:8]} vs {plan[c][:8]}"
    assert np.array_equal(sar.density_weights(S, S + 1), plan[S]) and np.array_equal(sar.density_weights(S, 0xFFFFFFFF), plan[S])


def test_smallest_plan_is_the_known_one(sar):
    assert sar.density_weights(2, 1).tolist() == [32768, 8192]


@ALL_S
def test_rows_sum_to_one(sar, S):
    offsets = _lattice(S)
    for c in range(1, S + 1):
        w = sar.density_weights(S, c)
        assert sum(int(w[dx * dx + dy * dy]) for dx, dy in offsets if dx * dx + dy * dy < S) == 65536, (S, c)


@ALL_S
def test_rows_fall_with_distance_and_vanish_where_dead(sar, S):
    for c in range(1, S + 1):
        w = sar.density_weights(S, c).astype(np.int64)
        live = np.arange(S) * c < S
        assert np.all(np.diff(w[live]) <= 0), (S, c)        # non-increasing in d2 over the live taps
        assert np.all(w[~live] == 0), (S, c)
        assert w[0] >= w[1 if S > 1 else 0] >= 0
        if c >= S:
            assert w[0] == 65536 and not w[1:].any()


@ALL_S
def test_rows_are_zero_exactly_where_dead_or_floored(sar, S):
    """Over the taps — the d2 some lattice offset of [-R, R]^2 has — a row is zero at every dead tap (d2 * c >= S), and a live tap is
    zero only where the contract's integer division floors it: (q[d2] << 16) < N, with q and N recomputed here. Every live tap has
    q >= 2^20 / S^2 >= 16 (u >= 1 / S), so nothing else can make one vanish. The issue's prototype already allows for such taps
    ("W_c[0] >= W_c[1] >= 0", and d2 = 1 is live in every class below S): none at S = 2, 5 and 64; at S = 256 there are 13, in 9 of the
    255 classes — (class, d2): (1, [241, 242, 244, 245, 250]), (2, [125]), (3, [85]), (5, [50]), (7, [36]), (14, [18]), (15, [17]),
    (51, [5]), (255, [1]); by hand, class 255: q[1] = floor((1/256)^2 * 2^20) = 16, N = 2^20 + 4 * 16, W[1] = 1048576 / 1048640 = 0."""
    offsets = _lattice(S)
    taps = np.array(sorted({dx * dx + dy * dy for dx, dy in offsets if dx * dx + dy * dy < S}))
    for c in range(1, S + 1):
        w = sar.density_weights(S, c)
        if c >= S:
            assert w[0] == 65536 and not w[1:].any(), (S, c)
            continue
        q = {}
        for d2 in (int(t) for t in taps if t * c < S):
            u = np.float64(1.0) - np.float64(d2 * c) / np.float64(S)
            q[d2] = int(np.floor(u * u * np.float64(1048576.0)))
            assert q[d2] >= 16, (S, c, d2)
        N = sum(q[dx * dx + dy * dy] for dx, dy in offsets if (dx * dx + dy * dy) * c < S)
        for d2 in (int(t) for t in taps):
            if d2 * c >= S:
                assert w[d2] == 0, f"S {S} class {c}: dead tap {d2} has weight {w[d2]}"
            elif d2:
                assert (w[d2] == 0) == ((q[d2] << 16) < N), f"S {S} class {c}: tap {d2} weight {w[d2]}, q {q[d2]}, N {N}"
            else:
                assert w[0] > 0, (S, c)


@ALL_S
def test_radius(sar, S):
    r = sar.density_radius(S)
    assert r == D.radius(S) and r * r <= S - 1 < (r + 1) * (r + 1)


def test_radius_of_the_named_sizes(sar):
    assert (sar.density_radius(64), sar.density_radius(256), sar.density_radius()) == (7, 15, 7)


def test_default_is_64(sar):
    assert sar.density_params().samples == 64


@pytest.mark.parametrize("S", [0, 1, 257])
def test_samples_out_of_range_are_refused(sar, S):
    with pytest.raises(sar.SarError):
        sar.density_radius(S)
    with pytest.raises(sar.SarError):
        sar.density_weights(S, 1)
    import ctypes as C
    lib = sar.load_library()
    p = sar.density_params(samples=S)
    assert lib.sar_runtime_density(None, C.byref(p), None) == 1     # SAR_ERR_INVALID before the runtime is looked at
    assert "samples" in lib.sar_last_error().decode()


def test_class_zero_and_null_runtime_are_refused(sar):
    with pytest.raises(sar.SarError):
        sar.density_weights(64, 0)
    assert sar.load_library().sar_runtime_density(None, None, None) == 1
    with pytest.raises(AttributeError):
        sar.density_params(sample=3)


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
@ALL_S
def test_mass_is_conserved_in_q16_away_from_the_border(S):
    R, rng = D.radius(S), np.random.default_rng(S)
    h, w = 45, 67
    count = np.zeros((h, w), dtype=np.uint32)
    inner = (rng.integers(0, 2 * S + 1, size=(h - 2 * R, w - 2 * R)) * (rng.random((h - 2 * R, w - 2 * R)) < 0.3)).astype(np.uint32)
    count[R:h - R, R:w - R] = inner
    _, _, _, st = D.filter(count, rng.random((h, w)), S)
    assert st["mass_in"] == int(inner.sum()) and st["mass_q16"] == st["mass_in"] << 16


def test_mass_leaves_through_the_border():
    count = np.zeros((9, 9), dtype=np.uint32)
    count[0, 0] = 1
    _, _, _, st = D.filter(count, np.zeros((9, 9)), 64)
    assert 0 < st["mass_q16"] < 65536


@ALL_S
def test_count_follows_the_lattice_symmetries(S):
    rng = np.random.default_rng(100 + S)
    count = (rng.integers(0, 2 * S + 1, size=(33, 31)) * (rng.random((33, 31)) < 0.3)).astype(np.uint32)
    steps = rng.random((33, 31))
    want = D.filter(count, steps, S)[0]
    for f in (np.rot90, np.fliplr, np.flipud, np.transpose):
        got = D.filter(np.ascontiguousarray(f(count)), np.ascontiguousarray(f(steps)), S)[0]
        assert np.array_equal(got, f(want)), f.__name__


@pytest.mark.parametrize("name", K.select("identity_all_bright"))
def test_identity_case(name):
    k, r = K.case(name), K.reference(name)
    assert np.array_equal(r.count, k.count) and np.array_equal(K.bits(r.steps), K.bits(k.steps))
    assert r.max == int(k.count.max()) and r.stats["spread"] == 0 and r.stats["mass_q16"] == r.stats["mass_in"] << 16
    assert np.array_equal(r.count2, k.count) and np.array_equal(K.bits(r.steps2), K.bits(k.steps))


@pytest.mark.parametrize("name", K.select("saturating_pixel_in_ones", "67x45"))
def test_saturation(name):
    k, r = K.case(name), K.reference(name)
    assert r.stats["saturated"] == 1 and r.count[k.height // 2, k.width // 2] == 0xFFFFFFFF and r.max == 0xFFFFFFFF


@pytest.mark.parametrize("name", K.select("steps_lone_"))
def test_a_pixel_nothing_reaches_keeps_its_hue_bits(name):
    k, r = K.case(name), K.reference(name)
    y, x = k.height // 2, k.width // 2
    assert K.bits(r.steps)[y, x] == K.bits(k.steps)[y, x]


def test_hue_is_the_mass_weighted_mean():
    count = np.zeros((5, 5), dtype=np.uint32)
    count[2, 1], count[2, 3] = 1, 1
    steps = np.zeros((5, 5))
    steps[2, 1], steps[2, 3] = 0.25, 0.75
    c, s, _, _ = D.filter(count, steps, 64)
    assert s[2, 2] == 0.5 and 0.25 < s[2, 1] < 0.5 < s[2, 3] < 0.75
