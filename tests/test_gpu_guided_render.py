"""Guided renders in the wavefront renderer (crt_renderer_set_guiding): image bits, the eight RayStats and — under adaptive
stopping — the per-pixel sample counts equal the guiding-aware forward integrator tests/guided_pt/guided_pt.c, which is the
oracle's forward mode where no field is bound or the field is untrained (tests/test_guided_render.py) and reaches the
field through the host-compiled device source. The CPU half — the restatement against the oracle, the independent field,
unbiasedness, the launch plan — is tests/test_guided_render.py and tests/test_guided_plan.py."""
import numpy as np
import pytest

import guided_render_cases as rc
import guided_render_common as cm
import seam_integrator as si
from guided_render_common import same_bits, stats_tuple

pytestmark = pytest.mark.gpu
u32 = np.uint32
CRT_ERR_UNSUPPORTED = -5


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("guided_render")


_BUILT, _TRUTH = {}, {}


def built(crt, name):
    if name not in _BUILT:
        _BUILT[name] = cm.Built(crt, rc.CASES[name])
    return _BUILT[name]


def device_renderer(crt, b, field="own", monkeypatch=None):
    """A Renderer of the case's scene with the case's field bound ("own"), another GuidingField, or none (None)."""
    case, desc = b.case, b.desc
    if monkeypatch is not None:
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)
    scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], case.depth, s["frame"], s["strategy"], s["filter"], s["filter_radius"],
                                  float(case.variance), case.min_spp if case.min_spp is not None else s["min_spp"])
    r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
    r._protos = protos
    if field is not None:
        r.set_guiding(b.lib_field(crt) if isinstance(field, str) else field)
    return r, mats


def run(crt, r, case, batches=None):
    import torch
    if case.variance > 0:
        r.render_adaptive(case.spp, batch=case.batch)
    else:
        s = 0
        for n in (batches or [case.spp]):
            r.render_samples(s, n)
            s += n
    torch.cuda.synchronize()
    return r


def device_render(crt, b, field="own", batches=None, monkeypatch=None):
    r, _ = device_renderer(crt, b, field, monkeypatch)
    return run(crt, r, b.case, batches)


def truth(crt, work, name):
    """The restatement's render of a case, computed once per module: (image, counts, stats tuple, coverage)."""
    if name not in _TRUTH:
        b = built(crt, name)
        hooks = None
        if b.case.mapped_dome:
            # The oracle's light functions know no mapped dome, so on this one case light_sample / light_pdf / light_escaped
            # of the truth are answered by the device's shading seam (crt_light_*_n): truth and kernel then share one
            # implementation of the light — as tests/test_gpu_volume_render.py does, and acceptable for its reason: that
            # seam is pinned elsewhere, bit for bit, to the numpy restatement of the reference's environment map
            # (tests/test_gpu_environment.py::test_light_functions_equal_the_restatement, tests/test_environment.py).
            _scene, mats, _p = crt.usda.build_world(b.desc, crt, crt.default_material)
            hooks = si.SeamHost(None, si.DeviceShade(crt, mats, b.desc.lights)).hooks
        _TRUTH[name] = cm.restatement(crt, work, b, light_hooks=hooks)
    return _TRUTH[name]


def compare(name, r, want):
    img, counts, st, _cov = want
    dst = stats_tuple(r.stats())
    print(name, "device", dst, "restatement", st)
    assert dst == st, (name, dst, st)
    dimg = r.image()
    bad = np.argwhere(dimg.view(u32) != img.view(u32))
    assert bad.shape[0] == 0, (name, bad.shape[0], bad[:3], dimg[tuple(bad[0][:2])] if len(bad) else None, img[tuple(bad[0][:2])] if len(bad) else None)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_guided_render_equals_the_restatement(crt, oracle, work, monkeypatch, name):
    want = truth(crt, work, name)
    b = built(crt, name)
    r = device_render(crt, b, monkeypatch=monkeypatch)
    pipe = r.pipeline()
    assert pipe["guiding"] and not pipe["fused"] and not pipe["shade_pipe"] and not pipe["camera_trace"] and not pipe["volumes"], pipe
    print(name, want[3])
    compare(name, r, want)
    if b.case.variance > 0:
        counts = want[1]
        dc = np.zeros(counts.size, u32)
        dc[r.pixel_indices()] = r.sample_counts()
        assert np.array_equal(dc.reshape(counts.shape), counts), name
        assert counts.min() < counts.max(), "the stopping rule fired somewhere and not everywhere"


def test_the_image_is_really_guided(crt, oracle):
    """The test that cannot pass without the feature: a bound, trained field changes the image."""
    b = built(crt, "room_power")
    bound, plain = device_render(crt, b), device_render(crt, b, field=None)
    assert bound.pipeline()["guiding"] and not plain.pipeline()["guiding"]
    assert np.isfinite(bound.image()).all()
    assert (bound.image().view(u32) != plain.image().view(u32)).any()


def test_detached_and_untrained_give_the_never_bound_image(crt, oracle):
    import torch
    b = built(crt, "room_power")
    plain = device_render(crt, b, field=None)
    r = device_render(crt, b)
    guided = r.image()
    r.set_guiding(None)
    r.clear()
    r.render_samples(0, b.case.spp)
    torch.cuda.synchronize()
    assert not r.pipeline()["guiding"]
    assert same_bits(r.image(), plain.image()) and stats_tuple(r.stats()) == stats_tuple(plain.stats())
    assert not same_bits(guided, plain.image())
    k = built(crt, "room_untrained")  # (k): bound, never trained
    u = device_render(crt, k)
    assert u.pipeline()["guiding"]
    assert same_bits(u.image(), plain.image()) and stats_tuple(u.stats()) == stats_tuple(plain.stats())


def test_batches_and_lanes_change_no_bit(crt, oracle, monkeypatch):
    b = built(crt, "room_power")
    monkeypatch.setenv("CRT_LANES", "1")
    one = device_render(crt, b)
    assert one.lanes() == 1
    split = device_render(crt, b, batches=[4, 12])
    assert same_bits(one.image(), split.image()) and stats_tuple(one.stats()) == stats_tuple(split.stats())
    monkeypatch.setenv("CRT_LANES", "3")
    monkeypatch.setenv("CRT_LANE_MIN_PATHS", "1")
    lanes = device_render(crt, b)
    assert lanes.lanes() == 3 and lanes.pipeline()["guiding"]
    assert same_bits(one.image(), lanes.image()) and stats_tuple(one.stats()) == stats_tuple(lanes.stats())


def test_an_update_between_batches_is_seen_by_the_next_batch(crt, oracle, work):
    """field.update between two render calls: the next batch is the restatement's render on the NEW image."""
    import torch
    b = built(crt, "room_power")
    g = b.lib_field(crt, upto=1)
    r, _ = device_renderer(crt, b, field=g)
    r.render_samples(0, 4)
    torch.cuda.synchronize()
    old = r.image()
    assert same_bits(old, cm.restatement(crt, work, b, image=g.image_bytes(), spp=4)[0])
    for samples, it in b.passes[1:]:
        g.update(samples, it)
    r.clear()
    r.render_samples(0, 4)
    torch.cuda.synchronize()
    want = cm.restatement(crt, work, b, image=g.image_bytes(), spp=4)
    assert same_bits(r.image(), want[0]) and stats_tuple(r.stats()) == want[2]
    assert not same_bits(r.image(), old)


def test_the_renderer_keeps_a_freed_field(crt, oracle, work):
    """crt_guiding_free of a bound field drops the caller's reference only: the next render is clean and still guided."""
    import torch
    b = built(crt, "room_power")
    g = b.lib_field(crt)
    image = g.image_bytes()
    r, _ = device_renderer(crt, b, field=g)
    g.close()
    run(crt, r, b.case)
    torch.cuda.synchronize()
    compare("room_power", r, cm.restatement(crt, work, b, image=image))
    r.set_guiding(None)  # the last reference goes here


def test_refusals_with_a_field_bound(crt, oracle):
    b = built(crt, "room_power")
    r, _ = device_renderer(crt, b)
    L = crt.lib()
    vol = crt.volumes.Volumes([crt.volumes.region(half_extent=1.0, sigma_s=1.0, sigma_a=0.5)])
    assert L.crt_renderer_set_volumes(r.h, vol.h) == CRT_ERR_UNSUPPORTED and "guiding" in crt.lib().crt_last_error().decode()
    ft = crt.textures.FaceTextures([])
    assert L.crt_renderer_set_face_textures(r.h, ft.h) == CRT_ERR_UNSUPPORTED and "guiding" in crt.lib().crt_last_error().decode()
    st = (crt.CrtTravStats * 2)()
    assert L.crt_render_samples_stats(r.h, 0, 1, None, st) == CRT_ERR_UNSUPPORTED and "guided" in crt.lib().crt_last_error().decode()
    r.set_guiding(None)
    assert L.crt_render_samples_stats(r.h, 0, 1, None, st) == 0
    # symmetric: a bound aggregate refuses the field
    r.set_volumes(vol)
    g = b.lib_field(crt)
    assert L.crt_renderer_set_guiding(r.h, g.h) == CRT_ERR_UNSUPPORTED and "volume" in crt.lib().crt_last_error().decode()
    r.set_volumes(None)
    r.set_face_textures(ft)
    assert L.crt_renderer_set_guiding(r.h, g.h) == CRT_ERR_UNSUPPORTED and "texture" in crt.lib().crt_last_error().decode()
    r.set_face_textures(None)
    assert L.crt_renderer_set_guiding(r.h, g.h) == 0
