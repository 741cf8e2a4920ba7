"""The renderer's launch plan WITHOUT a GPU: plan_launches (crust-render_amd/csrc/launch_plan.h) decides once per batch
which kernel instances run it; kernels/pathtrace.hip only looks the named instances up in its table, render.cpp loops. Here the
function is compiled as plain C++ (tests/launch_plan/plan_sweep.cpp, own main) and run as a child process.

The property sweep: for every engine outcome select_engine gives over the scene grid (direct leaves, packets, LDS
split, tree size, nine cold masks, root, four CRT_WIDE requests), the material table, the lights, derived records, the
stats build, CRT_FUSED and the batch size are crossed fully with (a) strategy x tail x depth x CRT_NOCLASSIFY_FROM, (b)
the seven switches that gate the shade instance, (c) the camera form's and the root cull's gates — 13 to 16 million plans
per build-switch tuple. (The full cross product of all 27 axes is 10^11 cases; the groups are the axes the function reads
together.) Each plan must name only instances the build holds, pass engine_accepts per traversal instance with that
instance's own cold bits, and keep the structural rules stated once in plan_sweep.cpp's check_case.

The decision table: tests/golden/launch_plan_cases.npz holds 6 304 input rows and what the ladder macros that
render_lane consisted of before the plan existed launched for them — that code, compiled with the launch macro
redefined to record the kernel expression, run once per row (one row per engine outcome x material table x lights x stats
x batch size, and every other input varied one at a time around one scene per engine class). The plan must reproduce
every row. Not in the table: a simple-material table on a curve image, which crt_renderer_new never forms (curve images
get the general instances) — the old combined check let its k_path without the curve arm through, the plan refuses it,
and the sweep asserts that this is the only kind of input the per-instance check refuses beyond the combined one."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "launch_plan", "plan_sweep.cpp")
TUPLES = {  # build-switch tuple -> (flags, instances the build holds)
    "default": ([], 66),
    "nopk": (["-DCRT_NOPK_BUILD=1"], 70),
    "no_wide_direct": (["-DCRT_WIDE_DIRECT_BUILD=0"], 62),
    "no_cam_compact": (["-DCRT_CAM_COMPACT_BUILD=0"], 66),
}


def build(tmp, name, flags):
    out = str(tmp / ("plan_sweep_" + name))
    res = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, SRC, "-o", out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return out


def sanitizers_present(tmp):
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp / "probe")],
                          capture_output=True).returncode == 0


@pytest.mark.parametrize("name", list(TUPLES))
def test_every_plan_of_the_sweep_keeps_the_rules(tmp_path, name):
    flags, n_keys = TUPLES[name]
    exe = build(tmp_path, name, ["-O2"] + flags)
    res = subprocess.run([exe, "sweep"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got = dict(t.split("=") for t in res.stdout.split())
    assert int(got["keys"]) == n_keys
    assert int(got["cases"]) > 10_000_000 and int(got["planned"]) > 10_000_000
    assert int(got["planned"]) + int(got["refused"]) == int(got["cases"])
    assert int(got["engines"]) >= 90 and int(got["noengine"]) > 0  # the grid reaches refusals of select_engine too
    if name == "default":  # the figures the sweeps that share the grid pin too (test_face_plan.py, test_volume_render.py)
        assert (int(got["engines"]), int(got["cases"])) == (120, 16312320), got


def test_the_plan_reproduces_the_decision_table_of_the_ladders(tmp_path):
    z = np.load(os.path.join(ROOT, "tests", "golden", "launch_plan_cases.npz"))
    inputs, want, names, fields = z["inputs"], z["decisions"], [str(n) for n in z["names"]], [str(f) for f in z["decision_fields"]]
    assert len(inputs) == len(want) > 6000
    # the table run is small: under the sanitizers where the compiler has their runtimes
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitizers_present(tmp_path) else ["-O1"]
    exe = build(tmp_path, "table", flags)
    text = "\n".join(" ".join(str(int(x)) for x in row) for row in inputs) + "\n"
    res = subprocess.run([exe, "table"], input=text, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(inputs)
    named = set()
    for k, (line, w) in enumerate(zip(lines, want)):
        if w[0] < 0:
            expect = "refused"
        else:
            vals = [names[v] if f in ("path", "extend", "shade", "shade_last", "shadow") else str(int(v)) for f, v in zip(fields, w)]
            named.update(v for v in vals if v.startswith("k_"))
            expect = " ".join(f"{f}={v}" for f, v in zip(fields, vals))
        assert line == expect, (k, inputs[k].tolist(), line, expect)
    assert len(named) == 66  # the table exercises every instance of the default build
