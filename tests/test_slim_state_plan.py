"""The slim path state's rule WITHOUT a GPU (crust-render_amd/csrc/launch_plan.h: plan_launches, LaunchPlan::slim_state,
table_has_no_emitter): tests/launch_plan/slim_sweep.cpp compiled as plain C++ and run as a child process.

The pipelined shade kernel's launches hand each other a 48-byte path state where the plan says so. The sweep crosses what
decides it — an emitter in the table or none, lights, the material table's kind (simple / general / with media) and size,
CRT_SHADE_PIPE, CRT_NOCLASSIFY_FROM, the stats build, CRT_FUSED, the batch size, the tail, the depth, derived records —
over every engine outcome of a scene grid, and plans each case with CRT_SLIM_STATE 0 and 1:
  * every field the plan held before is equal under both (so the knob can only change which form the kernel carries);
  * with the knob 0 the form is off; with it 1 the form is on exactly where the plan names the pipelined instance AND
    nothing in the table emits, and the instance it names is one the build holds, with the same DRV argument;
  * table_has_no_emitter: a colour with luminance 0, a luminance without colour and a black Emissive do not emit; any
    NaN, an infinity under a product, a product that would merely underflow, and a coloured Emissive count as emitters."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "launch_plan", "slim_sweep.cpp")


def test_the_slim_form_follows_the_pipelined_instance_and_the_emitters(tmp_path):
    exe = str(tmp_path / "slim_sweep")
    res = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got = {k: int(v) for k, v in (t.split("=") for t in res.stdout.split())}
    assert got["cases"] > 500_000 and got["planned"] > 100_000
    assert 0 < got["slim"] < got["piped"] < got["planned"]  # the form is on somewhere, off somewhere the instance runs
    assert got["slim_stats"] > 0                            # the stats build runs the pipelined instance, and the form with it
