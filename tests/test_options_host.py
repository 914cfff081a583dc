"""CPU: what sar_runtime_set_option and sar_runtime_set_test_option answer — status and sar_last_error text — for every option name
with every boundary value, for names of the other entry point and for unknown names, held line for line to the record of the
library before the options came from one table (tests/golden/option_replies.json, recorded by tests/golden/make_option_replies.py
at the parent commit). tests/c/sar_options.cpp makes the calls on a runtime object that never saw a device. No device needed."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "option_replies.json")


def _recipe():
    spec = importlib.util.spec_from_file_location("make_option_replies", os.path.join(ROOT, "tests", "golden", "make_option_replies.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_every_option_answers_as_recorded(sar, tmp_path):
    from strange_attractor_renderer_amd import _abi
    golden = json.load(open(GOLDEN))
    got = _recipe().replies(ROOT, tmp_path)
    assert list(got) == list(golden)
    for key in golden:
        assert got[key] == golden[key], key
    # the names the product entry point accepts for at least one value are the stable options, no more, no less
    sent = {key.split()[1] for key in got if key.startswith("option ")}
    accepted = {key.split()[1] for key, calls in got.items() if key.startswith("option ") and any(status == _abi.SAR_OK for _, status, _ in calls)}
    assert accepted == set(_abi.STABLE_OPTIONS)
    # ... and a test-hook name went to it and was refused
    assert "path" in sent - accepted
