"""The vertex function k_shade_pipe's vertex step and k_camera_vertex share (kernels/vertex_simple.hip.h) WITHOUT a GPU:
compiled as host C++ behind the stand-in for the HIP names (profiles/host_shade/) and run as a stand-alone program under
ASan + UBSan on 100 000 random first vertices — a camera path's constants as literals — through both material views. Every
result is compared bit for bit with the vertex put together from mat_scatter as the shading seam drives it
(kernels/shade_seam.hip) and the record's emission; the depth-limit arm is checked beside it. CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++")
def test_the_vertex_function_equals_the_seam_on_first_vertices_and_is_clean_under_asan_and_ubsan(tmp_path):
    env = dict(os.environ, TMPDIR=str(tmp_path))
    res = subprocess.run(["bash", os.path.join(ROOT, "profiles", "host_shade", "run_vertex.sh")], capture_output=True, text=True,
                         timeout=900, env=env)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    line = [l for l in res.stdout.splitlines() if l.startswith("vertices ")][-1].split()
    got = dict(vertices=int(line[1]), alive=int(line[3]), emitting=int(line[5]), depth=int(line[7]))
    assert got["vertices"] == 200000 and got["depth"] == 100000
    assert 100000 < got["alive"] < got["vertices"]        # most scatter; Emissive records and grazing samples do not
    assert 10000 < got["emitting"] < 90000                # emission taken at the first vertex, and records without any
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
