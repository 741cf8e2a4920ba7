"""The launch plan of textured renders and the binding entry point, without a GPU: plan_launches with PlanInputs::faces over
plan_sweep.cpp's grid (tests/launch_plan/faces_sweep.cpp), and crt_renderer_set_face_textures's argument check. That a
plan with faces off is the plan made before the input existed is pinned by tests/test_launch_plan.py, unchanged."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_plan_with_faces_keeps_the_rules(tmp_path):
    """With faces on: always per stage — no fused kernel, no tail — no camera-trace, camera-vertex or pixel-table launch, no
    pipelined or slim shade, raw material records, the FACES extend key (the engine width the image runs, the cold state
    with u, v) and the FACES shade key; the stats build and faces beside volumes refused, and nothing else that the image
    did not refuse already. With faces off: no textured form in any plan."""
    out = str(tmp_path / "faces_sweep")
    src = os.path.join(ROOT, "tests", "launch_plan", "faces_sweep.cpp")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    counts = dict(kv.split("=") for kv in run.stdout.split())
    assert int(counts["cases"]) > 10 ** 6 and int(counts["planned"]) > 0, counts
    assert counts["refused"] == counts["stats_refused"], counts  # textures refuse the stats build and nothing else
    assert counts["volumes_refused"] == counts["cases"], counts  # ... and never run beside volumes
    assert counts["shade_keys"] == "12", counts
    # the grid is plan_sweep.cpp's (tests/launch_plan/sweep_common.h, sweep_grid): the base sweep's figures, which
    # tests/test_launch_plan.py pins for its default tuple
    assert (int(counts["engines"]), int(counts["cases"])) == (120, 16312320), counts


def test_set_face_textures_is_declared_exported_and_checks_its_renderer(crt):
    assert "crt_renderer_set_face_textures" in crt.ABI_SYMBOLS_FACE_TEXTURES and hasattr(crt.lib(), "crt_renderer_set_face_textures")
    header = open(os.path.join(ROOT, "include", "crt_face_textures.h")).read()
    assert "int crt_renderer_set_face_textures(CrtRenderer *r, CrtFaceTextures *ft);" in header
    ft = crt.textures.FaceTextures([])
    assert crt.lib().crt_renderer_set_face_textures(None, ft.h) == -1  # CRT_ERR_BAD_ARG
    assert crt.lib().crt_renderer_set_face_textures(None, None) == -1
    ft.close()  # the caller's reference was the only one
