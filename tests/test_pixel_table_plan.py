"""The per-pixel camera table's rule WITHOUT a GPU (crust-render_amd/csrc/launch_plan.h: plan_launches,
LaunchPlan::pixel_table): tests/launch_plan/pixel_table_sweep.cpp compiled as plain C++ and run as a child process.

Where the plan says so, the camera launch (k_camera or k_camera_vertex) reads what a sample owes to its pixel alone from
the table the renderer filled at creation. The sweep crosses what decides it — the engine outcome of a scene grid, the
material table, lights, the stats build, CRT_FUSED, the depth, CRT_CAM_COMPACT, CRT_ROOT_CULL, a volume render, a partial
active list, CRT_SHADE_PIPE, motion, a lens, CRT_SLIM_STATE, CRT_CAMERA_VERTEX, CRT_CAMERA_TRACE 0 .. 3 and unset, and
whether the renderer holds a table — and plans each case with CRT_PIXEL_TABLE 0, 1 and unset:
  * every field the plan held before is equal under all three (the knob can only add the form);
  * with the knob 0 the form is off; with 1 or unset it is on exactly where a camera launch runs and a table exists —
    which implies every owned pixel sampling and a static pinhole batch, what the table's form of the sample relies on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "launch_plan", "pixel_table_sweep.cpp")


def test_the_pixel_table_follows_its_rule_and_moves_no_earlier_field(tmp_path):
    exe = str(tmp_path / "pixel_table_sweep")
    res = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got = {k: int(v) for k, v in (t.split("=") for t in res.stdout.split())}
    assert got["cases"] > 1_000_000 and got["planned"] > 200_000
    assert 0 < got["on"] < got["planned"] and got["unready"] > 0      # on somewhere; a camera launch without a table elsewhere
    assert got["on_vertex"] > 0 and got["on_trace"] > 0               # behind either camera launch
    assert got["on_modes"] > 0                                        # under the camera trace's test forms
    assert got["root_lds"] > 0                                        # CRT_CULL_ROOT_LDS follows its rule
