"""CPU: the Python parameter builders (search_params .. color_range_params) and the public record dtypes against
tests/golden/python_params.json, a record of the code BEFORE the builders were rewritten over one struct filler
(tests/golden/make_python_params.py writes it; run that at the parent commit of a change to the builders).

Every recorded row is one call: the tree under test must give the same struct bytes, or raise the same exception class. The rows
under "tightened" are the calls the recorded code let through and the filler's one rule refuses; each carries its reason and expects
ValueError. The dtypes are held to the recorded literals (names, formats, shapes, offsets, item size) both as the package exports
them and as numpy derives them from the _abi structures. No device needed."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_python_params as M  # noqa: E402

GOLDEN = json.load(open(M.GOLDEN))


def _rows(kind, builder):
    return [r for r in GOLDEN[kind] if r["builder"] == builder]


def test_the_golden_file_holds_the_table(sar):
    """the recorded calls are the generator's table, no more and no fewer; only marked rows are tightened, all to ValueError"""
    from strange_attractor_renderer_amd import _abi
    table = {(b, label): (kwargs, reason) for b, label, kwargs, reason in M.table(_abi)}
    recorded = GOLDEN["rows"] + GOLDEN["tightened"]
    assert sorted((r["builder"], r["label"]) for r in recorded) == sorted(table)
    for r in recorded:
        assert json.loads(json.dumps(table[r["builder"], r["label"]][0])) == r["kwargs"], (r["builder"], r["label"])
    for r in GOLDEN["rows"]:
        assert ("bytes" in r) != ("raises" in r)
    for t in GOLDEN["tightened"]:
        assert t["reason"] == table[t["builder"], t["label"]][1] and t["reason"] in (M.NON_INTEGRAL, M.SHADE_RANGE)
        assert t["raises"] == "ValueError" and t["recorded"] != {"raises": "ValueError"}
    assert sorted(GOLDEN["dtypes"]) == sorted(M.DTYPES)


@pytest.mark.parametrize("builder", list(M.BUILDERS))
def test_builder_gives_what_the_parent_gave(sar, builder):
    rows = _rows("rows", builder)
    assert rows and rows[0]["label"] == "defaults" and "bytes" in rows[0]
    wrong = []
    for r in rows:
        want = {k: r[k] for k in ("bytes", "raises") if k in r}
        got = M.outcome(sar, builder, r["kwargs"])
        if got != want:
            wrong.append((r["label"], got, want))
    assert not wrong, wrong


@pytest.mark.parametrize("builder", sorted({t["builder"] for t in GOLDEN["tightened"]}))
def test_builder_refuses_what_was_tightened(sar, builder):
    wrong = [(t["label"], got) for t in _rows("tightened", builder)
             if (got := M.outcome(sar, builder, t["kwargs"])) != {"raises": t["raises"]}]
    assert not wrong, wrong


@pytest.mark.parametrize("name", list(M.DTYPES))
def test_dtype_is_the_parents_and_the_abis(sar, name):
    from strange_attractor_renderer_amd import _abi
    lit = GOLDEN["dtypes"][name]
    want = M.dtype_of(lit)
    assert lit["abi"] == M.DTYPES[name]
    for got in (getattr(sar, name), np.dtype(getattr(_abi, lit["abi"]))):
        assert got == want and got.names == want.names and got.itemsize == want.itemsize
        assert M.dtype_literal(got) == {k: lit[k] for k in ("fields", "itemsize")}
