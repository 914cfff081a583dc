"""CPU: the exact Lyapunov references (tests/lyapunov_reference.py) on maps with known answers, then the search's numpy
restatement (tests/search_restatement.py, the GPU search's bit-for-bit yardstick) against both references. No device needed.

Tolerance: 1e-12 absolute on each exponent and on their sum. The restatement is fp64; against the 50-digit references it was
within 3e-13 on the conjugated Jordan block (a defective eigenvalue: the most sensitive case here), within 4e-15 on the other
affine maps and within 4e-16 for the sum rule on the seed-1 candidates below. A wrong norm, a missing rejection or a wrong
Jacobian entry moves an exponent by 1e-4 or more.
"""
import math

import numpy as np
import pytest

import lyapunov_reference as L
import search_restatement as R

TOL = 1e-12
NOLIMIT = dict(min_lyapunov=-math.inf, min_ky_dim=-math.inf, keep_rejected=True)


def test_diagonal_maps_give_log_of_the_diagonal():
    for d in ((0.5, -0.25, 0.9), (1.3, 0.01, -2.0), (0.75, 0.75, 0.75)):
        lam, ky = L.affine_spectrum([[d[0], 0, 0], [0, d[1], 0], [0, 0, d[2]]], 200)
        want = sorted((math.log(abs(v)) for v in d), reverse=True)
        assert lam == pytest.approx(want, rel=0, abs=1e-15)
        assert ky == L.ky_dimension(want)


def test_upper_triangular_leaves_the_frame_at_the_identity():
    A = [[0.9, 0.7, -0.4], [0.0, -0.5, 1.1], [0.0, 0.0, 0.3]]
    n = 300
    prod, q = L.affine_gram_schmidt(A, n)
    for k in range(3):          # column k of Q is +-e_k, whatever the signs of the diagonal did to it
        for i in range(3):
            assert abs(float(q[k][i])) == (1.0 if i == k else 0.0), (k, i, q[k][i])
        assert float(L._CTX.ln(prod[k])) / n == pytest.approx(math.log(abs(A[k][k])), rel=0, abs=1e-15)


def test_a_rotation_block_gives_two_equal_exponents():
    lam, ky = L.affine_spectrum(L.rotation_scaling(0.8, 0.9, 0.4), 500)
    assert lam[0] == pytest.approx(math.log(0.8), rel=0, abs=1e-15) and lam[1] == pytest.approx(lam[0], rel=0, abs=1e-15)
    assert lam[2] == pytest.approx(math.log(0.4), rel=0, abs=1e-15) and ky == 0.0
    # conjugated, the block is no longer a rotation: the two exponents split at finite N but keep their sum
    lam_c, _ = L.affine_spectrum(L.conjugate(L.rotation_scaling(0.8, 0.9, 0.4)), 500)
    assert abs(lam_c[0] - lam_c[1]) > 1e-4
    det = math.log(0.8 * 0.8 * 0.4)
    assert sum(lam_c) == pytest.approx(det, rel=0, abs=1e-14)


def test_kaplan_yorke_definition():
    assert L.ky_dimension([0.1, -0.05, -0.2]) == 2 + 0.05 / 0.2
    assert L.ky_dimension([0.1, -0.3, -0.4]) == 1 + 0.1 / 0.3
    assert L.ky_dimension([-0.1, -0.3, -0.4]) == 0.0
    assert L.ky_dimension([0.2, 0.1, -0.1]) == 3.0
    assert L.ky_dimension([0.2, 0.0, -0.4]) == 2 + 0.2 / 0.4


def test_the_reference_tells_a_finite_n_jordan_block_from_its_eigenvalue():
    lam, _ = L.affine_spectrum(L.AFFINE_MAPS["jordan_block"][0], 1500)
    assert all(abs(v - math.log(0.9)) > 5e-4 for v in (lam[0], lam[2]))     # the finite-N spread around log 0.9
    assert sum(lam) == pytest.approx(3 * math.log(0.9), rel=0, abs=1e-12)


@pytest.mark.parametrize("name", sorted(L.AFFINE_MAPS))
@pytest.mark.parametrize("steps", [1000, 1500])
def test_restatement_meets_the_decimal_reference_on_affine_maps(name, steps):
    A, b = L.AFFINE_MAPS[name]
    c = L.affine_coeffs(A, b)
    start, transient = (0.05, 0.05, 0.05), 200
    alive, status, done, _ = L.orbit_fate(c, start, transient, steps, L.AFFINE_BOUND)
    assert alive
    recs, _ = R.search(0, 0, 1, transient=transient, steps=steps, bound=L.AFFINE_BOUND, start=start, coeffs=np.array([c]),
                       **NOLIMIT)
    r = recs[0]
    assert (int(r["status"]), int(r["steps_done"])) == (status, done)
    folded = done if status == L.BOUNDED else done - 1
    lam, ky = L.affine_spectrum(A, folded)
    assert np.max(np.abs(np.array(r["lyapunov"]) - lam)) <= TOL, (r["lyapunov"], lam)
    assert abs(r["ky_dim"] - ky) <= TOL


def test_the_expanding_map_leaves_the_box_where_the_orbit_says():
    A, b = L.AFFINE_MAPS["complex_pair_expanding"]
    _, status, done, _ = L.orbit_fate(L.affine_coeffs(A, b), (0.05,) * 3, 200, 1500, L.AFFINE_BOUND)
    assert status == L.DIVERGED and 1000 < done < 1500


SUM_RULE_SEED, SUM_RULE_CANDIDATES = 1, (545, 1791, 2513, 2573, 2617)   # accepted at 4000 steps (min_lyapunov 0.005)


def test_restatement_meets_the_sum_rule_on_found_maps():
    steps, transient, start, bound = 4000, 1000, (0.05, 0.05, 0.05), 1e6
    cs = np.concatenate([R.candidates(SUM_RULE_SEED, k, 1) for k in SUM_RULE_CANDIDATES])
    recs, stats = R.search(0, 0, len(cs), transient=transient, steps=steps, coeffs=cs, min_lyapunov=0.005)
    assert stats["accepted"] == len(SUM_RULE_CANDIDATES)
    for r, c in zip(recs, cs):
        alive, status, done, p0 = L.orbit_fate(list(c), start, transient, steps, bound)
        assert alive and (int(r["status"]), int(r["steps_done"])) == (status, done) == (L.BOUNDED, steps)
        want = L.log_det_sum(list(c), p0, steps) / steps
        assert abs(math.fsum(r["lyapunov"]) - want) <= TOL, (r["candidate"], math.fsum(r["lyapunov"]), want)
