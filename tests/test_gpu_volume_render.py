"""Volume regions in the wavefront renderer (crt_renderer_set_volumes): image bits, the eight RayStats and — under adaptive
stopping — the per-pixel sample counts equal the volume-aware forward integrator tests/volume_pt/volume_pt.c, which is
the oracle's forward mode where no region is crossed (tests/test_volume_render.py) and reaches the walks through the
host-compiled device source. The CPU half — the restatement against the oracle, the independent walks, the physics, the
launch plan — is tests/test_volume_render.py."""
import os

import numpy as np
import pytest

import ora
import ora_world
import seam_integrator as si
import volume_pt as vp
import volume_ref as vr
import volume_render_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32 = np.uint32
CRT_ERR_UNSUPPORTED = -5


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("volume_render")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(u32), np.ascontiguousarray(b).view(u32))


def stats_tuple(st):
    return tuple(int(getattr(st, f)) for f, _t in ora.RayStats._fields_)


def device_renderer(crt, case, regions="own"):
    """A Renderer of the case's scene with the case's regions bound ("own"), other regions, or none (None)."""
    desc = case.desc
    scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], case.depth, s["frame"], s["strategy"], s["filter"], s["filter_radius"],
                                  float(case.variance), case.min_spp if case.min_spp is not None else s["min_spp"])
    r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
    r._protos = protos
    if regions is not None:
        r.set_volumes(crt.volumes.Volumes(case.regions if regions == "own" else regions))
    return r, mats


def device_render(crt, case, regions="own", batches=None):
    import torch
    r, _mats = device_renderer(crt, case, regions)
    if case.variance > 0:
        r.render_adaptive(case.spp, batch=case.batch)
    else:
        s = 0
        for n in (batches or [case.spp]):
            r.render_samples(s, n)
            s += n
    torch.cuda.synchronize()
    return r


_TRUTH = {}


def truth(crt, work, name):
    """The restatement's render of a case, computed once per module: (case, image, counts, stats tuple, coverage)."""
    if name not in _TRUTH:
        case = rc.CASES[name](crt)
        o = ora_world.OracleRenderer(case.desc, crt.usda, max_depth=case.depth)
        vol = crt.volumes.Volumes(case.regions)
        hooks, threads = None, None
        if case.mapped_dome:
            # The oracle's light functions know no mapped dome, so on this one case light_sample / light_pdf / light_escaped
            # of the truth are answered by the device's shading seam (crt_light_*_n): truth and k_volume then share one
            # implementation of the light. Acceptable only because that seam is pinned elsewhere, bit for bit, to the numpy
            # restatement of the reference's environment map: tests/test_gpu_environment.py::
            # test_light_functions_equal_the_restatement (and its CPU half, tests/test_environment.py).
            _scene, mats, _p = crt.usda.build_world(case.desc, crt, crt.default_material)
            hooks, threads = si.SeamHost(None, si.DeviceShade(crt, mats, case.desc.lights)).hooks, 1
        vi = vp.VolumeIntegrator(work, o, vp.host_table(vr.host(work), vol.image_bytes()), light_hooks=hooks)
        img, counts, st, cov = vi.render(case.spp, threads=threads, variance=case.variance, min_spp=case.min_spp)
        _TRUTH[name] = (case, img, counts, stats_tuple(st), cov)
    return _TRUTH[name]


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_volume_render_equals_the_restatement(crt, oracle, work, name):
    case, img, counts, st, cov = truth(crt, work, name)
    r = device_render(crt, case)
    pipe = r.pipeline()
    assert pipe["volumes"] and not pipe["fused"] and not pipe["root_cull"] and not pipe["shade_pipe"], pipe
    dst = stats_tuple(r.stats())
    print(name, "device", dst, "restatement", st, cov)
    assert dst == st, (name, dst, st)
    dimg = r.image()
    bad = np.argwhere(dimg.view(u32) != img.view(u32))
    assert bad.shape[0] == 0, (name, bad.shape[0], bad[:3], dimg[tuple(bad[0][:2])] if len(bad) else None, img[tuple(bad[0][:2])] if len(bad) else None)
    assert cov["phase_vertices"] > 0, (name, cov)  # every case scatters inside a region
    if case.variance > 0:
        dc = np.zeros(img.shape[0] * img.shape[1], u32)
        dc[r.pixel_indices()] = r.sample_counts()
        assert np.array_equal(dc.reshape(counts.shape), counts), name
        assert counts.min() < counts.max(), "the stopping rule fired somewhere and not everywhere"


def test_the_cases_cover_every_arm_of_the_volume_forward_form(crt, oracle, work):
    total = dict.fromkeys(rc.COVERAGE, 0)
    for name in sorted(rc.CASES):
        for k, v in truth(crt, work, name)[4].items():
            total[k] += v
    assert all(total[k] > 0 for k in rc.COVERAGE), total


@pytest.mark.parametrize("scene,depth", [("cornellbox", 8), ("veach_mis", 8)])
def test_an_uncrossed_aggregate_changes_no_bit(crt, scene, depth):
    """No-op identity: bound but never crossed, every new operation is absent — image and counters are those of the same
    renderer with nothing bound, and only the bound run reports the volume stage."""
    desc = crt.usda.load(rc.scene_file(scene), 40, 24)
    case = rc.Case(scene, desc, rc.far_away(crt.volumes), depth=depth)
    bound, plain = device_render(crt, case), device_render(crt, case, regions=None)
    assert bound.pipeline()["volumes"] and not plain.pipeline()["volumes"]
    assert stats_tuple(bound.stats()) == stats_tuple(plain.stats())
    assert same_bits(bound.image(), plain.image())
    empty = device_render(crt, case, regions=[])  # an empty aggregate
    assert empty.pipeline()["volumes"] and stats_tuple(empty.stats()) == stats_tuple(plain.stats()) and same_bits(empty.image(), plain.image())


def test_batches_and_lanes_change_no_bit(crt, monkeypatch):
    make = lambda: rc._smoke(w=96, h=54, spp=6)(crt)
    monkeypatch.setenv("CRT_LANES", "1")
    one = device_render(crt, make())
    assert one.lanes() == 1
    split = device_render(crt, make(), batches=[1, 5])
    assert same_bits(one.image(), split.image()) and stats_tuple(one.stats()) == stats_tuple(split.stats())
    monkeypatch.setenv("CRT_LANES", "3")
    monkeypatch.setenv("CRT_LANE_MIN_PATHS", "1")
    lanes = device_render(crt, make())
    assert lanes.lanes() == 3 and lanes.pipeline()["volumes"]
    assert same_bits(one.image(), lanes.image()) and stats_tuple(one.stats()) == stats_tuple(lanes.stats())


def test_two_runs_give_identical_bytes(crt):
    a = device_render(crt, rc.CASES["smoke_depth16"](crt))
    b = device_render(crt, rc.CASES["smoke_depth16"](crt))
    assert a.image().tobytes() == b.image().tobytes() and stats_tuple(a.stats()) == stats_tuple(b.stats())


def test_detach_gives_the_never_bound_image(crt):
    import torch
    case = rc.CASES["fog_depth8_power"](crt)
    r = device_render(crt, case)
    fogged = r.image()
    r.set_volumes(None)
    r.clear()
    r.render_samples(0, case.spp)
    torch.cuda.synchronize()
    plain = device_render(crt, case, regions=None)
    assert not r.pipeline()["volumes"]
    assert same_bits(r.image(), plain.image()) and stats_tuple(r.stats()) == stats_tuple(plain.stats())
    assert not same_bits(fogged, plain.image())


def test_the_stats_build_refuses_a_bound_renderer(crt):
    case = rc.CASES["fog_depth2"](crt)
    r, _ = device_renderer(crt, case)
    st = (crt.CrtTravStats * 2)()
    assert crt.lib().crt_render_samples_stats(r.h, 0, 1, None, st) == CRT_ERR_UNSUPPORTED
    r.set_volumes(None)
    assert crt.lib().crt_render_samples_stats(r.h, 0, 1, None, st) == 0


def test_render_with_report_binds_the_scene_regions_and_counts_them(crt):
    """render_with_report(..., volumes=True): the file's crust:volume prims become the bound aggregate, the report's
    "volume regions" row counts them, and the image is the fogged one."""
    path = rc.scene_file("fog")
    img, st = crt.render_with_report(path, spp=4, width=40, height=24, max_depth=4, variance=0.0, volumes=True)
    assert st.scene.volumes == 1
    assert any(line.split()[:2] == ["volume", "regions"] and line.split()[-1] == "1" for line in st.report().splitlines()), st.report()
    plain, st0 = crt.render_with_report(path, spp=4, width=40, height=24, max_depth=4, variance=0.0)
    assert st0.scene.volumes == 0 and "volume regions" not in st0.report()
    assert np.isfinite(img).all() and not same_bits(img, plain)
