"""The scenes of tests/media_cases.py on the device: 16 x 16 at the case's samples, frames 0..3, every strategy of the
case, through the default pipeline, CRT_FUSED=1, CRT_FUSED=0, one lane and three lanes (r.pipeline() says which form ran:
the fused kernel on the lightless and rect forms when asked for, the per-stage launches wherever the black dome stands).
The image bits and all eight RayStats equal the oracle's, and the closed-form bound of tests/test_media.py holds on the
device's own image.

Every scene here holds a medium, so every launch is a MATS == 2 instance; numbered_media gives k_number_media runs of
three records and a compact id (351) that differs from the material index (1 050); the last test asks for one medium more
than the 14-bit id can number."""
import numpy as np
import pytest

import media_cases as mc
from test_gpu_radiometry import COUNTERS, KNOBS, PIPELINES

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in mc.cases()}
FRAMES = 4
K_MAX_MEDIA = (1 << 14) - 1  # render_kernels.h
_oracle = {}


def oracle(case, strategy, frame):
    """The oracle's image and counters of one frame, rendered once for the five pipelines."""
    key = (case.name, strategy, frame)
    if key not in _oracle:
        import ora_world
        img, st = ora_world.OracleRenderer(case.build(strategy, frame), mc.usda).render(case.spp, forward=1)
        _oracle[key] = (img, tuple(int(getattr(st, f)) for f in COUNTERS))
    return _oracle[key]


def renderer(crt, desc):
    scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], s["max_depth"], s["frame"], s["strategy"], s["filter"],
                                  s["filter_radius"], 0.0)
    r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
    r._protos = protos
    return r, scene


def device(crt, desc, spp):
    import torch
    r, scene = renderer(crt, desc)
    r.render_samples(0, spp)
    torch.cuda.synchronize()
    st = r.stats()
    scene.traversal_error()
    return r.image(), tuple(int(getattr(st, f)) for f in COUNTERS), r.pipeline(), r.lanes()


def set_pipeline(monkeypatch, pipeline):
    env, fused, lanes = PIPELINES[pipeline]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return fused, lanes


@pytest.mark.parametrize("pipeline", list(PIPELINES))
@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_the_oracle_and_the_closed_form(crt, monkeypatch, name, pipeline):
    case = CASES[name]
    fused, lanes = set_pipeline(monkeypatch, pipeline)
    truth = case.truth()
    for s in case.strategies:
        means = []
        for frame in range(FRAMES):
            desc = case.build(s, frame)
            img, counters, pipe, ran_lanes = device(crt, desc, case.spp)
            want_img, want_counters = oracle(case, s, frame)
            assert counters == want_counters, (name, s, frame, dict(zip(COUNTERS, zip(counters, want_counters))))
            bad = np.argwhere(img.view(np.uint32) != want_img.view(np.uint32))
            assert bad.shape[0] == 0, (name, s, frame, bad.shape[0], bad[:3])
            # no fused instance carries a light at infinity: the dome forms run per stage whatever is asked for; the
            # lightless and rect forms run the fused MEDIA instance when it is asked for
            at_infinity = any(l["kind"] in ("dome", "distant") for l in desc.lights)
            if fused is not None:
                assert pipe["fused"] is (fused and not at_infinity), (name, pipeline, pipe)
            elif at_infinity:
                assert pipe["fused"] is False, (name, pipeline, pipe)
            assert lanes is None or ran_lanes == lanes, (name, pipeline, ran_lanes)
            assert counters[COUNTERS.index("camera_rays")] == mc.W * mc.H * case.spp
            means.append(case.reduce(img))
        mean, se = mc.mean_and_se(np.array(means))
        print("%s %s %s: mean %s truth %s rel %s, 5 SE %.2e" % (name, pipeline, s, mean, truth, mean / truth - 1.0,
                                                                5.0 * (se / truth).max()))
        assert np.all(np.abs(mean - truth) <= 5.0 * se + case.allowance(s) * truth), (name, s, mean, truth, se)


@pytest.mark.parametrize("pipeline", ["fused", "per_stage"])
@pytest.mark.parametrize("depth", [3, 8])
def test_chromatic_slab_on_the_device_is_the_oracles(crt, monkeypatch, depth, pipeline):
    """The conservative chromatic slab of test_media.py (multiple scattering, roulette, chromatic weights) on the device:
    bits and counters, and each channel against the device's own grey render within 5 sqrt(SE_a^2 + SE_b^2)."""
    set_pipeline(monkeypatch, pipeline)
    chroma, greys = mc.chromatic_vs_grey(depth)
    est = []
    for case in [chroma] + greys:
        means = []
        for frame in range(FRAMES):
            img, counters, _pipe, _lanes = device(crt, case.build("power", frame), case.spp)
            want_img, want_counters = oracle(case, "power", frame)
            assert counters == want_counters, (case.name, frame, dict(zip(COUNTERS, zip(counters, want_counters))))
            assert np.array_equal(img.view(np.uint32), want_img.view(np.uint32)), (case.name, frame)
            means.append(case.reduce(img))
        est.append(mc.mean_and_se(np.array(means)))
    (mean, se) = est[0]
    for c, (gm, gs) in enumerate(est[1:]):
        assert abs(mean[c] - gm[c]) <= 5.0 * np.hypot(se[c], gs[c]), (depth, c, mean[c], gm[c], se[c], gs[c])


def test_one_medium_too_many_is_refused_and_the_process_renders_on(crt, monkeypatch):
    """kMaxMedia + 1 = 16 384 media-bearing materials: the compact id has 14 bits, 0 meaning none, so renderer creation is
    refused with an exception; the same process then renders clear_normal_d2 as the oracle does."""
    set_pipeline(monkeypatch, "default")
    desc = mc.too_many_media(K_MAX_MEDIA + 1)
    assert len(desc.geoms) >= K_MAX_MEDIA + 1
    with pytest.raises(crt.CrtError):
        renderer(crt, desc)
    fits, _scene = renderer(crt, mc.too_many_media(K_MAX_MEDIA))  # the same scene with one fewer is accepted
    assert fits.h
    case = CASES["clear_normal_d2"]
    img, counters, _pipe, _lanes = device(crt, case.build("power", 0), case.spp)
    want_img, want_counters = oracle(case, "power", 0)
    assert counters == want_counters and np.array_equal(img.view(np.uint32), want_img.view(np.uint32))
