"""scenes/face_textured.usda end to end on the device's seam functions: the reference integrator (the oracle's scalar
trace_path) with crt_intersect1 for the kernel seam, crt_face_resolve_n for the face lookup and
crt_material_scatter_faces_n / _eval_faces_n for the textured shading (face_seam_host.DeviceFaces over the aggregate
usda.build_face_textures made), against the same integrator on the oracle's traversal and untextured functions with
tests/face_ref.py choosing the base colour (RefFaces): image and all eight RayStats counters, bit for bit, at 40 x 24,
4 samples, depth 8, forward = 1. Two cases: the scene as it stands (a placement moves: rays carry a time) and with the
moving placement removed (has_motion false); the device run is repeated once for identical bits. One query per launch:
a case is one test, the device render is made once per case and shared."""
import numpy as np
import pytest

import face_seam_host as fsh
import ora
import ora_world
import seam_integrator as si

pytestmark = pytest.mark.gpu
SPP, DEPTH = 4, 8


def device_host(crt, desc):
    scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
    ft = crt.usda.build_face_textures(desc, crt)
    shade = si.DeviceShade(crt, mats, desc.lights)
    host = fsh.FaceSeamHost(si.DeviceKernel(crt, scene), shade, fsh.DeviceFaces(crt, ft, shade.mats), desc)
    host.keep = (scene, protos, ft)
    return host, scene


@pytest.fixture(scope="module")
def cases(crt, oracle, tmp_path_factory):
    """case -> (desc, oracle renderer, device host, device scene, device image, device counters), rendered on first use."""
    made = {}

    def get(case):
        if case not in made:
            desc = fsh.load_scene(crt, static_dir=tmp_path_factory.mktemp("static") if case == "static" else None)
            o = ora_world.OracleRenderer(desc, crt.usda, max_depth=DEPTH)
            assert (o.job.width, o.job.height) == (40, 24)
            host, scene = device_host(crt, desc)
            img, st = host.render(o, SPP, forward=1)
            assert host.errors == []
            made[case] = (desc, o, host, scene, img, st)
        return made[case]
    return get


@pytest.mark.parametrize("case", ["moving", "static"])
def test_host_integrator_on_the_textured_seam_matches_the_truth_image(crt, cases, case):
    desc, o, host, scene, img, st = cases(case)
    assert bool(scene.has_motion()) == (case == "moving")
    truth = fsh.truth_host(desc, o)
    want, want_st = truth.render(o, SPP, forward=1)
    assert truth.errors == []
    for f, _t in ora.RayStats._fields_:
        assert getattr(st, f) == getattr(want_st, f), (f, getattr(st, f), getattr(want_st, f))
    bad = np.argwhere(img.view(np.uint32) != want.view(np.uint32))
    assert bad.shape[0] == 0, (bad.shape[0], bad[:3])
    assert host.seen == truth.seen and all(n > 0 for n in host.seen.values()), host.seen
    # and the textures are in it: not the image of the authored colours
    plain, _ = o.render(SPP, threads=1, forward=1)
    assert (img.view(np.uint32) != plain.view(np.uint32)).any()


def test_a_second_device_run_gives_identical_bits(cases):
    _desc, o, host, _scene, img, st = cases("static")
    again, again_st = host.render(o, SPP, forward=1)
    assert host.errors == []
    assert np.array_equal(again.view(np.uint32), img.view(np.uint32))
    for f, _t in ora.RayStats._fields_:
        assert getattr(again_st, f) == getattr(st, f), f
