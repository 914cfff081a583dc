"""Exact references for the Lyapunov spectra of the chaotic-map search (include/sar.h: sar_runtime_search), written apart from
the search and its restatement (tests/search_restatement.py): standard library only.

1. affine_spectrum: for x' = A x + b the Jacobian is the constant A. The finite-N spectrum is the mean log of the modified
   Gram-Schmidt norms of A·Q over N steps, Q = I at the start, the columns taken in the order 1, 2, 3. It is computed here in
   `decimal` at 50 digits from the exact values of A's fp64 entries. (At finite N these are not log|eigenvalue|: a Jordan
   block's three exponents only approach log|eigenvalue| as N grows.)
2. log_det_sum: for any map the sum of the exponents times the folded steps is the sum over those steps of log|det J(p_t)|,
   whatever the frame Q does. The orbit p_t is stepped in plain Python floats (IEEE fp64, no fused operations, next_point's
   operation order, so the same points as the device's); each det J is exact (fractions.Fraction of the fp64 entries) and
   the logs are summed with math.fsum.
"""
from __future__ import annotations

import math
from decimal import Context, Decimal
from fractions import Fraction

BOUNDED, DIVERGED, DEGENERATE = 0, 1, 2
_CTX = Context(prec=50, Emin=-10**8, Emax=10**8)


def affine_coeffs(A, b=(0.0, 0.0, 0.0)) -> list:
    """The 30 coefficients of x' = A x + b: row r holds b[r] at 0 and A[r][0], A[r][1], A[r][2] at 1 (x), 5 (y), 8 (z)."""
    out = [0.0] * 30
    for r in range(3):
        out[10 * r + 0] = float(b[r])
        out[10 * r + 1], out[10 * r + 5], out[10 * r + 8] = (float(v) for v in A[r])
    return out


def next_point(c, x: float, y: float, z: float):
    """PolynomialSprott2Degree::next_point in fp64: c0 + x c1 + xx c2 + xy c3 + xz c4 + y c5 + yy c6 + yz c7 + z c8 + zz c9,
    added left to right."""
    terms = (x, x * x, x * y, x * z, y, y * y, y * z, z, z * z)
    out = []
    for r in range(3):
        s = c[10 * r]
        for k in range(9):
            s = s + terms[k] * c[10 * r + 1 + k]
        out.append(s)
    return out


def _within(p, bound: float) -> bool:
    return all(abs(v) <= bound for v in p)


def orbit_fate(coeffs, start, transient: int, steps: int, bound: float):
    """(survived the transient, status, steps_done, the point the Lyapunov phase starts from) for one map, from the fp64 orbit
    alone. A point leaving the box [-bound, bound]^3 (or NaN) ends the orbit: in the transient the candidate is dropped; at
    Lyapunov step t (0-based) the record is DIVERGED with steps_done = t + 1."""
    p = [float(v) for v in start]
    for _ in range(transient):
        p = next_point(coeffs, *p)
        if not _within(p, bound):
            return False, None, None, None
    p0 = list(p)
    for t in range(steps):
        p = next_point(coeffs, *p)
        if not _within(p, bound):
            return True, DIVERGED, t + 1, p0
    return True, BOUNDED, steps, p0


def ky_dimension(lam) -> float:
    """Kaplan-Yorke dimension of a descending spectrum: j the largest count with lam_1 + .. + lam_j >= 0, then
    j + (lam_1 + .. + lam_j) / |lam_{j+1}|; 0 if lam_1 < 0, 3 if all three partial sums are >= 0."""
    s, j = 0.0, 0
    for i in range(3):
        if s + lam[i] < 0.0:
            break
        s += lam[i]
        j = i + 1
    if j == 3:
        return 3.0
    return 0.0 if j == 0 else j + s / abs(lam[j])


def affine_gram_schmidt(A, folded: int):
    """(the product of each column's Gram-Schmidt norms, the final frame Q as its columns) after `folded` steps of
    V = A Q, then modified Gram-Schmidt of V's columns in the order 1, 2, 3, from Q = I; 50-digit decimal arithmetic, A's
    entries taken as the exact values of their fp64 numbers."""
    ctx = _CTX
    a = [[Decimal(float(A[r][k])) for k in range(3)] for r in range(3)]
    one, zero = Decimal(1), Decimal(0)
    q = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]      # q[k] is column k of Q
    prod = [one, one, one]                                             # one log per column at the end, not one per step

    def dot(u, v):
        return ctx.add(ctx.add(ctx.multiply(u[0], v[0]), ctx.multiply(u[1], v[1])), ctx.multiply(u[2], v[2]))

    for _ in range(folded):
        v = [[dot(a[r], q[k]) for r in range(3)] for k in range(3)]   # V = A Q, column by column
        for k in range(3):
            for j in range(k):                                         # reject column k against q_1 .. q_{k-1}, in turn
                d = dot(q[j], v[k])
                v[k] = [ctx.subtract(v[k][i], ctx.multiply(d, q[j][i])) for i in range(3)]
            n = ctx.sqrt(dot(v[k], v[k]))
            if n == 0:
                raise ZeroDivisionError("a column of A Q vanished: A is singular")
            prod[k] = ctx.multiply(prod[k], n)
            q[k] = [ctx.divide(w, n) for w in v[k]]
    return prod, q


def affine_spectrum(A, folded: int):
    """(exponents sorted descending, Kaplan-Yorke dimension) of the constant Jacobian A after `folded` Gram-Schmidt steps."""
    if folded <= 0:
        raise ValueError("no folded step: no exponents")
    prod, _ = affine_gram_schmidt(A, folded)
    lam = sorted((float(_CTX.divide(_CTX.ln(p), folded)) for p in prod), reverse=True)
    return lam, ky_dimension(lam)


def jacobian(c, x: float, y: float, z: float):
    """J of next_point at (x, y, z), each entry in fp64 as the search evaluates it: row r is
    (c1 + 2x c2 + y c3 + z c4,  x c3 + c5 + 2y c6 + z c7,  x c4 + y c7 + c8 + 2z c9)."""
    x2, y2, z2 = x + x, y + y, z + z
    J = []
    for r in range(3):
        k = c[10 * r:10 * r + 10]
        J.append((((k[1] + x2 * k[2]) + y * k[3]) + z * k[4],
                  ((x * k[3] + k[5]) + y2 * k[6]) + z * k[7],
                  ((x * k[4] + y * k[7]) + k[8]) + z2 * k[9]))
    return J


def _log_abs(f: Fraction) -> float:
    # math.log of Python ints is exact to rounding at any size: no underflow however small det J is
    return math.log(abs(f.numerator)) - math.log(f.denominator)


def log_det_sum(coeffs, p0, folded: int) -> float:
    """sum over t < folded of log|det J(p_t)|, p_0 = p0 and p_{t+1} = next_point(p_t); -inf if some det J is exactly 0."""
    p = [float(v) for v in p0]
    logs = []
    for _ in range(folded):
        J = [[Fraction(v) for v in row] for row in jacobian(coeffs, *p)]
        det = (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])
               + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))
        if det == 0:
            return -math.inf
        logs.append(_log_abs(det))
        p = next_point(coeffs, *p)
    return math.fsum(logs)


# ---- non-normal affine test maps: A = S B S^-1 ---------------------------------------------------------------------
def _mat_mul(a, b):
    return [[math.fsum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _mat_inv(a):
    f = [[Fraction(v) for v in row] for row in a]
    det = (f[0][0] * (f[1][1] * f[2][2] - f[1][2] * f[2][1]) - f[0][1] * (f[1][0] * f[2][2] - f[1][2] * f[2][0])
           + f[0][2] * (f[1][0] * f[2][1] - f[1][1] * f[2][0]))
    cof = [[(f[(j + 1) % 3][(i + 1) % 3] * f[(j + 2) % 3][(i + 2) % 3] - f[(j + 1) % 3][(i + 2) % 3] * f[(j + 2) % 3][(i + 1) % 3])
            for j in range(3)] for i in range(3)]
    return [[float(cof[i][j] / det) for j in range(3)] for i in range(3)]


SKEW = [[1.0, 0.6, -0.3], [0.2, 1.0, 0.5], [-0.4, 0.3, 1.0]]          # a basis far from orthogonal


def conjugate(B, S=SKEW):
    """S B S^-1 rounded to fp64: non-normal and not triangular for a generic S."""
    return _mat_mul(_mat_mul(S, B), _mat_inv(S))


def rotation_scaling(rho: float, theta: float, third: float):
    """B with the complex pair rho e^{+-i theta} in its upper 2x2 block and the real eigenvalue `third`."""
    c, s = rho * math.cos(theta), rho * math.sin(theta)
    return [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, third]]


def jordan(lam: float):
    """A single 3x3 Jordan block with eigenvalue lam."""
    return [[lam, 1.0, 0.0], [0.0, lam, 1.0], [0.0, 0.0, lam]]


def nearly_singular():
    """A with singular values ~1.19, ~0.75 and ~5e-9: a non-normal, non-triangular 2x2 block (complex pair 0.55 +- 0.40i)
    over the eigenvalue 1e-8. The plane z = 0 is invariant (row z is (0, 0, 1e-8)), so the third Gram-Schmidt column stays
    e_z and its norm is 1e-8 to the last bit, while the first two columns rotate. (For a generic S B S^-1 with an eigenvalue
    1e-8, fp64 Gram-Schmidt loses ~eps |A| / 1e-8 = 1e-8 of the third norm to cancellation every step: no fp64 search could
    meet an exact reference there, so such a map tests the arithmetic's conditioning, not the search.)"""
    return [[0.7, 0.9, 0.35], [-0.2, 0.4, -0.6], [0.0, 0.0, 1e-8]]


# name -> (A, b): the affine maps both the CPU and the GPU tests hold to affine_spectrum (tests/test_lyapunov_reference.py,
# tests/test_gpu_search.py)
AFFINE_MAPS = {
    "complex_pair_expanding": (conjugate(rotation_scaling(0.95, 0.7, 1.25)), (0.1, -0.2, 0.05)),
    "jordan_block": (conjugate(jordan(0.9)), (0.3, 0.1, -0.2)),
    "mixed_real": (conjugate([[0.8, 0.0, 0.0], [0.0, -0.6, 0.0], [0.0, 0.0, 0.05]]), (-0.1, 0.2, 0.4)),
    "nearly_singular": (nearly_singular(), (0.1, -0.2, 0.05)),
}
# the expanding map's orbit grows ~1.25x a step: inside 1e150 for 1000 steps, out of it (DIVERGED) before 1500
AFFINE_BOUND = 1e150
