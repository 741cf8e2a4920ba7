"""The camera-trace rule WITHOUT a GPU (crust-render_amd/csrc/launch_plan.h: plan_launches, LaunchPlan::camera_trace,
extend_deferred_key): tests/launch_plan/camera_sweep.cpp compiled as plain C++ and run as a child process.

Where the plan says so, one launch of k_camera generates, culls and traces a batch's camera rays and the first extend is
the k_extend_deferred instance over the rays it left. The sweep crosses what decides it — the engine outcome of a scene
grid (direct words, packets, tree size, cold state, the LDS split, a root or none, the CRT_WIDE requests), the material
table, lights and lights at infinity, lens, motion, CRT_CAM_COMPACT, CRT_ROOT_CULL, the stats build, CRT_FUSED, the batch
size, the depth, a volume render, a partial active list — and plans each case with CRT_CAMERA_TRACE 0, 1, 2, 3 and unset:
  * every field the plan held before is equal under all five (the knob can only add the form);
  * with the knob 0 the form is off; with 1, 2, 3 it is on exactly where the rule stated in the sweep holds, names the
    deferred instance with `extend`'s own arguments, an instance the build holds, and the test forms carry their mode;
  * unset, it is on only for trees of at most kCameraTraceMaxNodes nodes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "launch_plan", "camera_sweep.cpp")


def test_the_camera_trace_follows_its_rule_and_moves_no_earlier_field(tmp_path):
    exe = str(tmp_path / "camera_sweep")
    res = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got = {k: int(v) for k, v in (t.split("=") for t in res.stdout.split())}
    assert got["cases"] > 5_000_000 and got["planned"] > 1_000_000
    assert 0 < got["on_default"] < got["on"] < got["planned"]  # on somewhere, off elsewhere; large trees only when asked
    assert got["on_nocull"] > 0 and got["large_forced"] > 0   # with and without the root cull
