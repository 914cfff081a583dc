"""The reference side of the depth cases (tests/depth_cases.py), without a GPU: every case's condition on the C oracle at both
sizes — the case still reaches the state it was built for —, and the oracle against tests/golden/second_restatement.py on each
case's map, bit for bit: count, max, zbuf, steps, both colorize kinds and Runtime::merge. tests/test_gpu_depth_cases.py holds the
device to the oracle on the same cases."""
import os
import sys

import numpy as np
import pytest

import depth_cases as DC

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import second_restatement as R  # noqa: E402

SMALL, SMALL_JOBS = (48, 32), 3


@pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", DC.NAMES)
def test_the_case_reaches_its_state_on_the_oracle(oracle, case, size):
    f = DC.check_condition(oracle, case, size)
    print(f"{case} {size[0]}x{size[1]}: {f}")


def test_case_table_and_start_sets():
    assert len(DC.NAT) == 9 and set(DC.NAMES) - set(DC.NAT) == {"rising_tied", "falling_sentinel"}
    nat, tied, sentinel = (DC.start_set(s) for s in DC.START_SETS)
    assert nat.shape == (DC.JOBS, 3) and np.array_equal(nat[:, :2], tied[:, :2]) and np.array_equal(nat[:, :2], sentinel[:, :2])
    assert np.all(tied[:, 2] == 2.0 ** -5) and np.all(sentinel[1::2, 2] == 2.0 ** -6)
    assert np.array_equal(sentinel[0::2, 2], 0.2 * nat[0::2, 2])


def _same(a, b, what):
    """An oracle runtime against a restatement runtime, bit for bit."""
    assert np.array_equal(a.count.ravel(), np.array(b.count, dtype=np.uint32)) and a.max == b.max, f"{what}: count / max"
    assert np.array_equal(DC.bits(a.zbuf.ravel()), DC.bits(np.array(b.zbuf, dtype=np.float32))), f"{what}: zbuf"
    assert np.array_equal(DC.bits(a.steps.ravel()), DC.bits(np.array(b.steps, dtype=np.float64))), f"{what}: steps"


def _restated(case, starts, n):
    b = R.Runtime(*SMALL)
    for p0 in starts:
        R.render(DC.preset(case), b, tuple(float(v) for v in p0), n)
    return b


@pytest.mark.parametrize("case", DC.NAMES)
def test_oracle_agrees_with_the_second_restatement(oracle, case):
    """3 jobs at 48 x 32: the whole render, Depth and Gas colorize, and the merge of jobs {0, 1} with job {2}."""
    n = DC.CASES[case]["n"]
    st = DC.starts(case)[:SMALL_JOBS]
    a = DC.oracle_runtime(oracle, case, SMALL, 0, SMALL_JOBS)
    b = _restated(case, st, n)
    _same(a, b, f"{case}: render")
    assert np.count_nonzero(a.count) > 100, case
    ref = DC.freeze(oracle, case, SMALL, a)
    assert np.array_equal(ref.depth.reshape(-1, 4), np.array(R.colorize_depth(b), dtype=np.uint16)), f"{case}: Depth image"
    for transparent in (0, 1):
        assert np.array_equal(ref.gas[transparent].reshape(-1, 4),
                              np.array(R.colorize_gas(b, transparent=bool(transparent)), dtype=np.uint16)), f"{case}: Gas image"
    a1, a2 = DC.oracle_runtime(oracle, case, SMALL, 0, 2), DC.oracle_runtime(oracle, case, SMALL, 2, 3)
    b1, b2 = _restated(case, st[:2], n), _restated(case, st[2:], n)
    assert oracle.merge(a1, a2) == 0
    b1.merge(b2)
    _same(a1, b1, f"{case}: merge")
    _same(a1, b, f"{case}: merge against the sequential render")   # contiguous job slices folded in order
