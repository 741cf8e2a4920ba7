"""The camera-vertex rule WITHOUT a GPU (crust-render_amd/csrc/launch_plan.h: plan_launches, LaunchPlan::camera_vertex):
tests/launch_plan/camera_vertex_sweep.cpp compiled as plain C++ and run as a child process.

Where the plan says so, k_camera_vertex shades the first vertex of a camera path in the lane that traced its ray, and the
first extend and shade launches see only the rays it deferred. The sweep crosses what decides it — the engine outcome of a
scene grid, the material table and its size against the pipelined kernel's budget, lights, the stats build, CRT_FUSED, the
depth, CRT_CAM_COMPACT, CRT_ROOT_CULL, a volume render, a partial active list, CRT_SHADE_PIPE, CRT_SHADE_WIDE,
CRT_NOCLASSIFY_FROM, an emitter in the table, CRT_SLIM_STATE, CRT_CAMERA_TRACE 0, 2, 3 and unset — and plans each case
with CRT_CAMERA_VERTEX 0, 1 and unset:
  * every field the plan held before — the camera trace, its mode and the deferred instance included — is equal under all
    three (the knob can only add the form);
  * with the knob 0 the form is off; with 1 or unset it is on exactly where the camera trace holds, the early shade is
    the pipelined instance and the depth is at least 1; the camera trace's test forms keep their mode."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "launch_plan", "camera_vertex_sweep.cpp")


def test_the_camera_vertex_follows_its_rule_and_moves_no_earlier_field(tmp_path):
    exe = str(tmp_path / "camera_vertex_sweep")
    res = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got = {k: int(v) for k, v in (t.split("=") for t in res.stdout.split())}
    assert got["cases"] > 5_000_000 and got["planned"] > 1_000_000
    assert 0 < got["on"] < got["planned"] and got["trace_only"] > 0  # on somewhere; k_camera alone elsewhere
    assert got["on_slim"] > 0 and got["on_full"] > 0                 # survivors in the slim form and in the full one
    assert got["on_nocull"] > 0 and got["on_modes"] > 0              # without the root cull; under the test forms
