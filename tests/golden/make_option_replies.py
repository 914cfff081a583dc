"""Records what sar_runtime_set_option and sar_runtime_set_test_option answer, as tests/golden/option_replies.json:

    python tests/golden/make_option_replies.py PATH_TO_A_CHECKOUT_OF_THE_PARENT_COMMIT

Run it ON THE PARENT COMMIT of a change to the option code: the file is a record of the library BEFORE the change, which
tests/test_options_host.py replays against the tree under test, line for line. The checkout must be built (python -m
strange_attractor_renderer_amd.build); tests/c/sar_options.cpp of THIS tree is compiled against that checkout's private headers and
its hooks build. No device needed.

The file maps "entry point, option name" to the calls made with that name, in order: [value as a decimal string, status,
sar_last_error text] each."""
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "option_replies.json")
PROGRAM = os.path.join("tests", "c", "sar_options.cpp")


def replies(root, workdir):
    """builds tests/c/sar_options.cpp inside the tree `root` against root's hooks build, runs it and returns its rows"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(root, PROGRAM)
    if root != ROOT:  # (a parent checkout: THIS tree's program against that checkout's headers and library)
        shutil.copy(os.path.join(ROOT, PROGRAM), src)
    hooks = os.path.join(root, "tests", "hooks")
    exe = os.path.join(str(workdir), "sar_options")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-value", src, "-o", exe, "-L", hooks, "-l:libsar_hip_hooks.so",
                    f"-Wl,-rpath,{hooks}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)
    rows = [line.split("\t") for line in out.stdout.splitlines()]
    assert all(len(r) == 5 for r in rows), [r for r in rows if len(r) != 5][:3]
    table = {}
    for entry, name, value, status, text in rows:
        table.setdefault(f"{entry} {name}", []).append([value, int(status), text])
    return table


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        table = replies(os.path.abspath(sys.argv[1]), tmp)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()) + "\n}\n")
    print(f"{sum(len(v) for v in table.values())} calls under {len(table)} names recorded from {sys.argv[1]}")
