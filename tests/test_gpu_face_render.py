"""Textured renders in the wavefront renderer (crt_renderer_set_face_textures), bit for bit: scenes/face_textured.usda at
40 x 24, 4 spp, depth 8, forward = 1 — image and all eight RayStats counters of the renderer with the aggregate bound against
the FaceSeamHost run of the reference integrator (tests/face_seam_host.py), once on the CPU backend (the oracle's traversal
and untextured functions, face_ref choosing the base colour) and once on DeviceKernel + FacedMaterials; the case without the
moving placement (has_motion false: no time plane); two runs alike; and the unbound behaviour — the unbound renderer equals
today's oracle image, detaching restores it and drops | 512, binding beside volumes and the stats entry are refused."""
import numpy as np
import pytest

import face_seam_host as fsh
import ora
import ora_world
import seam_integrator as si

pytestmark = pytest.mark.gpu
SPP, DEPTH = 4, 8
UNSUPPORTED = -5


def make_renderer(crt, desc):
    scene, materials, protos = crt.usda.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], DEPTH, s["frame"], s["strategy"], s["filter"], s["filter_radius"], 0.0,
                                  s["min_spp"])
    r = crt.Renderer(scene, materials, desc.lights, crt.make_camera(**desc.camera), settings)
    r._protos = protos
    return r, scene, materials


def render(r):
    import torch
    r.clear()
    r.render_samples(0, SPP)
    torch.cuda.synchronize()
    return r.image(), r.stats()


def same_counters(a, b):
    for f, _t in ora.RayStats._fields_:
        assert getattr(a, f) == getattr(b, f), (f, getattr(a, f), getattr(b, f))


def same_bits(a, b):
    bad = np.argwhere(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))
    assert bad.shape[0] == 0, (bad.shape[0], bad[:3])


@pytest.fixture(scope="module")
def cases(crt, oracle, tmp_path_factory):
    """case -> dict(desc, o, r, scene, materials, ft, img, st): the bound renderer's picture, made on first use."""
    made = {}

    def get(case):
        if case not in made:
            desc = fsh.load_scene(crt, static_dir=tmp_path_factory.mktemp("static") if case == "static" else None)
            o = ora_world.OracleRenderer(desc, crt.usda, max_depth=DEPTH)
            assert (o.job.width, o.job.height) == (40, 24)
            r, scene, materials = make_renderer(crt, desc)
            ft = crt.usda.build_face_textures(desc, crt)
            r.set_face_textures(ft)
            img, st = render(r)
            assert r.pipeline()["face_textures"] and not r.pipeline()["fused"]
            made[case] = dict(desc=desc, o=o, r=r, scene=scene, materials=materials, ft=ft, img=img, st=st)
        return made[case]
    return get


@pytest.mark.parametrize("case", ["moving", "static"])
def test_bound_renderer_matches_the_host_integrator_truth(crt, cases, case):
    c = cases(case)
    assert bool(c["scene"].has_motion()) == (case == "moving")
    truth = fsh.truth_host(c["desc"], c["o"])
    want, want_st = truth.render(c["o"], SPP, forward=1)
    assert truth.errors == [] and all(n > 0 for n in truth.seen.values())
    same_counters(c["st"], want_st)
    same_bits(c["img"], want)


def test_bound_renderer_matches_the_host_integrator_on_the_device_seam(crt, cases):
    c = cases("moving")
    shade = si.DeviceShade(crt, c["materials"], c["desc"].lights)
    host = fsh.FaceSeamHost(si.DeviceKernel(crt, c["scene"]), shade, fsh.DeviceFaces(crt, c["ft"], shade.mats), c["desc"])
    want, want_st = host.render(c["o"], SPP, forward=1)
    assert host.errors == []
    same_counters(c["st"], want_st)
    same_bits(c["img"], want)


def test_two_bound_runs_give_identical_bits(cases):
    c = cases("static")
    img, st = render(c["r"])
    same_bits(img, c["img"])
    same_counters(st, c["st"])


def test_unbound_and_detached_renderers_are_todays(crt, cases):
    c = cases("static")
    want, want_st = c["o"].render(SPP, forward=1)  # today's oracle image: the authored colours
    fresh, _scene, _mats = make_renderer(crt, c["desc"])
    img, st = render(fresh)
    same_bits(img, want)
    same_counters(st, want_st)
    unbound_pipeline = fresh.pipeline()
    assert not unbound_pipeline["face_textures"]
    assert (c["img"].view(np.uint32) != img.view(np.uint32)).any()  # the bound picture is another one
    r = c["r"]
    try:
        r.set_face_textures(None)
        again, again_st = render(r)
        same_bits(again, img)
        same_counters(again_st, st)
        assert r.pipeline() == unbound_pipeline
    finally:
        r.set_face_textures(c["ft"])


def test_refusals_beside_volumes_and_for_the_stats_entry(crt, cases):
    c = cases("static")
    r, L = c["r"], crt.lib()
    vol = crt.volumes.Volumes([crt.volumes.region()])
    assert L.crt_renderer_set_volumes(r.h, vol.h) == UNSUPPORTED and "textures together with volumes" in L.crt_last_error().decode()
    with pytest.raises(crt.CrtError, match="CRT_ERR_UNSUPPORTED"):
        r.render_samples_stats(0, 1)
    other, _scene, _mats = make_renderer(crt, c["desc"])
    other.set_volumes(vol)
    assert L.crt_renderer_set_face_textures(other.h, c["ft"].h) == UNSUPPORTED
    assert "textures together with volumes" in L.crt_last_error().decode()
    other.set_volumes(None)
    other.set_face_textures(c["ft"])  # and once the volumes are gone it binds
    # a binding past the renderer's tables
    big = crt.textures.FaceTextures([], [crt.textures.FaceMap([0], [0])], [(len(c["desc"].geoms), 0, False)], [])
    assert L.crt_renderer_set_face_textures(other.h, big.h) == -1 and "the renderer has" in L.crt_last_error().decode()
