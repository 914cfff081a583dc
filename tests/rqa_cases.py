"""What the recurrence-analysis tests share (tests/test_rqa_host.py, tests/test_gpu_rqa.py): the random sets — a noisy cycle with
laminar stretches — and the shapes they are run at, the planted sets with their closed-form histograms, and every parameter set the
calls must refuse, with a piece of the message they leave."""
import math

import numpy as np

# The phases of one round of the noisy cycle: seven points, three of them held for 3, 2 and 4 steps. The round's period (13) puts
# long lines on the diagonals k = 13, 26, ..; the held phases put short ones on k = 1, 2, 3 and make the vertical lines longer than 1.
PHASES = np.array([0, 1, 1, 1, 2, 3, 3, 4, 5, 6, 6, 6, 6])
NOISE = 0.01
EPS2 = 0.03 * 0.03        # eps2 / (2 NOISE^2) = 4.5: two visits of one phase recur with probability 0.79 (chi-squared, 3 degrees)

# (T, jobs, sets, theiler, line_bins). With 256 diagonals to a band, 256 columns to a tile and 256 values of i to a chunk of a walk:
# T = 1, 2, 3 have no, one and two diagonals; 63, 64, 65 fewer diagonals than lanes; 255, 256, 257 (theiler 0) 254, 255 and 256 of
# them — one band to the last lane, exactly one band —, 257 with theiler 0 / 258 - 1 one band and a chunk's length +- 1; 511 and 513
# two and three bands, an even and an odd number to fold; 700 three bands with a tail, and a column tile's tail. theiler = T - 1
# leaves nothing.
SHAPES = [
    (1, 3, 1, 0, 256), (2, 1, 3, 0, 4), (2, 3, 1, 1, 2), (3, 3, 3, 0, 256), (3, 1, 1, 1, 4),
    (63, 3, 1, 0, 256), (64, 1, 3, 1, 4), (65, 3, 3, 5, 256), (65, 1, 1, 64, 256),
    (255, 1, 1, 0, 256), (256, 3, 1, 0, 2), (257, 1, 3, 0, 256), (257, 3, 1, 1, 256), (256, 1, 1, 255, 4),
    (511, 1, 3, 5, 256), (513, 3, 1, 0, 4), (513, 1, 1, 1, 256), (700, 3, 3, 0, 256), (700, 1, 1, 5, 2),
]


def noisy_cycle(t, jobs=1, sets=1, seed=7):
    """(sets, jobs * t, 3): every trajectory walks PHASES from a random offset around seven points of the unit cube, NOISE added."""
    rng = np.random.default_rng(seed + 1000 * t + 10 * jobs + sets)
    base = rng.random((7, 3))
    out = np.zeros((sets, jobs, t, 3))
    for s in range(sets):
        for j in range(jobs):
            phase = PHASES[(np.arange(t) + rng.integers(0, PHASES.size)) % PHASES.size]
            out[s, j] = base[phase] + NOISE * rng.standard_normal((t, 3))
    return out.reshape(sets, jobs * t, 3)


def _empty(line_bins):
    return np.zeros(line_bins + 1, dtype=np.uint64), np.zeros(line_bins + 1, dtype=np.uint64)


def _counts(t, w, rec, diag_lengths, vert_lengths):
    return dict(recurrences=rec, pairs=(t - w - 1) * (t - w) // 2 if t > w + 1 else 0, diag_lines=len(diag_lengths),
                vert_lines=len(vert_lengths), diag_longest=max(diag_lengths, default=0), vert_longest=max(vert_lengths, default=0))


def _histograms(diag_lengths, vert_lengths, line_bins):
    diag, vert = _empty(line_bins)
    for l in diag_lengths:
        diag[min(l, line_bins)] += 1
    for l in vert_lengths:
        vert[min(l, line_bins)] += 1
    return diag, vert


def constant_lines(t, w, line_bins):
    """T equal points: everything outside the Theiler band recurs. Diagonal k > w is one line of T - k; column j has the runs
    j - w (above the band) and T - 1 - j - w (below it) where positive."""
    dl = [t - k for k in range(w + 1, t)]
    vl = [l for j in range(t) for l in (j - w, t - 1 - j - w) if l > 0]
    return _histograms(dl, vl, line_bins) + (_counts(t, w, sum(dl), dl, vl),)


def tiled_lines(t, p, w, line_bins):
    """p distinct far-apart points tiled to T (w < p): i and j recur where p divides j - i. The lines lie on k = p, 2p, .. with length
    T - k; every vertical line has length 1, and column j has one for every other i of its residue."""
    assert w < p
    dl = [t - k for k in range(p, t, p)]
    vl = [1] * (2 * sum(dl))
    return _histograms(dl, vl, line_bins) + (_counts(t, w, sum(dl), dl, vl),)


def tiled_points(t, p):
    """p points a distance of at least 1 apart, tiled to T."""
    base = np.zeros((p, 3))
    base[:, 0] = np.arange(p)
    base[:, 1] = np.arange(p) % 2
    return base[np.arange(t) % p]


def planted_sets():
    """name -> (points (T, 3), parameters of recurrence_lines): what the arithmetic must get right at the edges."""
    inf = math.inf
    infs = np.zeros((9, 3))
    infs[[1, 4, 6], 0] = inf          # inf - inf = NaN: not recurrent with each other; inf - 0 = inf: not recurrent with the rest
    infs[3, 1] = -inf
    sub = np.zeros((8, 3))
    sub[:, 0] = [0.0, 5e-324, 1e-170, -1e-170, 1e-162, 3e-162, 1.0, 1.0 + 2.0 ** -52]      # r2 underflows to 0 (recurrent), or is tiny
    zeros = np.zeros((6, 3))
    zeros[::2] = -0.0
    lattice = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0],
                        [0.0, 1.0, 0.0]])
    return {
        "infinities": (infs, dict(eps2=1.0, line_bins=4)),
        "subnormals": (sub, dict(eps2=5e-324, line_bins=4)),
        "subnormals, eps2 1e-320": (sub, dict(eps2=1e-320, line_bins=4)),
        "minus zero": (zeros, dict(eps2=1e-300, line_bins=8)),
        "lattice, eps2 = 1": (lattice, dict(eps2=1.0, line_bins=8)),                        # distance exactly 1 is not below 1
        "lattice, eps2 = 1 + ulp": (lattice, dict(eps2=math.nextafter(1.0, 2.0), line_bins=8)),
    }


# recurrence_lines: changes to (n=12, samples=0, theiler=0, line_bins=4, chunk=0, eps2=1.0)
RECURRENCE_REFUSED = [
    (dict(n=0), "2^20 points"), (dict(n=2 ** 20 + 1), "2^20 points"),
    (dict(samples=5), "samples must divide"), (dict(samples=24), "samples must divide"),
    (dict(line_bins=0), "line_bins"), (dict(line_bins=1), "line_bins"), (dict(line_bins=4097), "line_bins"),
    (dict(eps2=0.0), "eps2"), (dict(eps2=-1.0), "eps2"), (dict(eps2=math.inf), "eps2"), (dict(eps2=math.nan), "eps2"),
    (dict(chunk=2 ** 30 + 1), "chunk"),
]

# recurrence_plot on 12 points as 2 trajectories of 6: changes to (job=0, window=(0, 0, 6, 6))
PLOT_REFUSED = [
    (dict(job=2), "trajectories"), (dict(window=(0, 0, 0, 6)), "2^24 pixels"), (dict(window=(0, 0, 6, 0)), "2^24 pixels"),
    (dict(window=(1, 0, 6, 6)), "leaves the trajectory"), (dict(window=(0, 1, 6, 6)), "leaves the trajectory"),
    (dict(window=(6, 0, 1, 1)), "leaves the trajectory"), (dict(window=(0, 2 ** 32 - 1, 1, 2)), "leaves the trajectory"),
]

# recurrence_analysis: changes to (jobs=2, samples=8, stride=1, transient=10, bound=1e6)
RQA_REFUSED = [
    (dict(jobs=0), "jobs must be"), (dict(jobs=2 ** 16 + 1, samples=1), "jobs must be"),
    (dict(samples=0), "at least 1"), (dict(stride=0), "at least 1"),
    (dict(jobs=1025, samples=1024), "2^20 points"),
    (dict(transient=2 ** 31 + 1), "at most 2^31"),
    (dict(bound=0.0), "bound"), (dict(bound=math.inf), "bound"), (dict(bound=math.nan), "bound"),
    (dict(line_bins=1), "line_bins"), (dict(line_bins=4097), "line_bins"),
    (dict(chunk=2 ** 30 + 1), "chunk"),
    (dict(eps2=-1.0), "eps2"), (dict(eps2=math.inf), "eps2"), (dict(eps2=math.nan), "eps2"),
    (dict(eps_fraction=0.0), "eps_fraction"), (dict(eps_fraction=math.inf), "eps_fraction"), (dict(eps_fraction=math.nan), "eps_fraction"),
]
