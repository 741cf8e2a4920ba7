"""The launch plan of guided renders and the binding entry point, without a GPU: plan_launches with PlanInputs::guided over
plan_sweep.cpp's grid (tests/launch_plan/guided_sweep.cpp), the new header's one declaration, its export, and the argument
checks that need no device. That a plan with guided off is the plan made before the input existed is pinned by
tests/test_launch_plan.py, unchanged."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_plan_with_guided_keeps_the_rules(tmp_path):
    """With guided on: always per stage — no fused kernel, no tail — no compact camera paths, no camera-trace, camera-vertex
    or pixel-table launch, no pipelined or slim shade, the GUIDED shade key (k_shade_vol's twelve rows), extend and shadow
    the unbound per-stage plan's; the stats build, volumes and textures refused, and nothing else that the image did not
    refuse already. With guided off: no guided form in any plan (that it is the parent's plan field for field is
    tests/test_launch_plan.py's golden file, made before the input existed)."""
    out = str(tmp_path / "guided_sweep")
    src = os.path.join(ROOT, "tests", "launch_plan", "guided_sweep.cpp")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    counts = dict(kv.split("=") for kv in run.stdout.split())
    assert int(counts["cases"]) > 10 ** 6 and int(counts["planned"]) > 0, counts
    assert counts["refused"] == counts["stats_refused"] and int(counts["stats_refused"]) > 0, counts  # the stats build, and nothing else
    assert counts["volumes_refused"] == counts["cases"] == counts["faces_refused"], counts  # never beside volumes or textures
    assert counts["shade_keys"] == "12", counts
    # the grid is plan_sweep.cpp's (tests/launch_plan/sweep_common.h, sweep_grid): the base sweep's figures, which
    # tests/test_launch_plan.py pins for its default tuple
    assert (int(counts["engines"]), int(counts["cases"])) == (120, 16312320), counts


def test_the_header_declares_one_entry_point_and_it_is_exported(crt):
    header = open(os.path.join(ROOT, "include", "crt_render_guiding.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = re.findall(r"\b(crt_\w+)\s*\(", code)
    assert decls == ["crt_renderer_set_guiding"], decls
    assert "int crt_renderer_set_guiding(CrtRenderer *r, CrtGuiding *g);" in code
    assert crt.ABI_SYMBOLS_RENDER_GUIDING == ["crt_renderer_set_guiding"] and hasattr(crt.lib(), "crt_renderer_set_guiding")
    out = subprocess.run(["nm", "-D", "--defined-only", crt.lib()._name], capture_output=True, text=True, timeout=120).stdout
    assert re.search(r" T crt_renderer_set_guiding$", out, flags=re.M)
    # the two headers it stands beside keep their declarations: crt_guiding.h still declares its nine
    gh = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crt_guiding.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(crt_\w+)\s*\(", gh))) == sorted(crt.ABI_SYMBOLS_GUIDING)


def test_the_argument_checks_need_no_device(crt):
    """What can be asked without a device: the NULL renderer. The symmetric refusals (a field beside volumes or textures, and
    the reverse) need a CrtRenderer, and crt_renderer_new uploads its tables: no renderer exists without a device, so they run
    in tests/test_gpu_guided_render.py; on the plan they are checked above for every case of the grid. The CRT_REGEN_FIRST
    refusal belongs to an A/B build of the library that no test here compiles — as for set_volumes and set_face_textures."""
    g = crt.guiding.GuidingField([-1, -1, -1], [1, 1, 1])
    L = crt.lib()
    assert L.crt_renderer_set_guiding(None, g.h) == -1  # CRT_ERR_BAD_ARG
    assert L.crt_renderer_set_guiding(None, None) == -1
    g.close()  # the caller's reference was the only one


def test_usda_load_path_guiding_still_only_reads_settings(crt):
    """usda.load(path_guiding=True) stays a reader of settings: it hands back the configuration and binds nothing."""
    desc = crt.usda.load(os.path.join(ROOT, "scenes", "cornellbox_guided.usda"), 24, 16, path_guiding=True)
    assert not hasattr(desc, "guiding_field")
    assert "crt_renderer_set_guiding" not in open(os.path.join(ROOT, "crust-render_amd", "usda.py")).read()
