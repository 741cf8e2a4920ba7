"""The scenes of tests/radiometry_cases.py on the device: 16 x 16 at 64 spp, frames 0..3, every strategy of the case,
through the default pipeline, CRT_FUSED=1, CRT_FUSED=0, one lane and three lanes (r.pipeline() says which form ran: the
fused kernel on the lightless interiors, the per-stage launches wherever a light at infinity stands). The image bits and all
eight RayStats equal the oracle's, and the closed-form bound of tests/test_radiometry.py holds on the device's own image.

These are shapes no other GPU test has: one analytic sphere seen from inside, an emissive material that also scatters,
specular_weight 0, a black dome beside an area light, a sphere light cut by the horizon."""
import numpy as np
import pytest

import ora
import radiometry_cases as rc

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in rc.cases()}
FRAMES = 4
COUNTERS = [f for f, _t in ora.RayStats._fields_]
KNOBS = ("CRT_FUSED", "CRT_STAGE_MIN_PATHS", "CRT_PREFER_STAGE", "CRT_LANES", "CRT_LANE_MIN_PATHS", "CRT_WIDE", "CRT_SHADE_PIPE",
         "CRT_ROOT_CULL", "CRT_CAM_COMPACT", "CRT_GRID_MULT", "CRT_CAMERA_TRACE", "CRT_CAMERA_VERTEX", "CRT_PIXEL_TABLE",
         "CRT_SLIM_STATE")
# name: (environment, fused as r.pipeline() must report it or None, lanes as r.lanes() must report them or None)
PIPELINES = {"default": ({}, None, None),
             "fused": ({"CRT_FUSED": "1"}, True, None),
             "per_stage": ({"CRT_FUSED": "0"}, False, None),
             "one_lane": ({"CRT_LANES": "1", "CRT_LANE_MIN_PATHS": "1"}, None, 1),
             "three_lanes": ({"CRT_LANES": "3", "CRT_LANE_MIN_PATHS": "1"}, None, 3)}
_oracle = {}


def oracle(case, strategy, frame):
    """The oracle's image and counters of one frame, rendered once for the five pipelines."""
    key = (case.name, strategy, frame)
    if key not in _oracle:
        import ora_world
        img, st = ora_world.OracleRenderer(case.build(strategy, frame), rc.usda).render(rc.SPP, forward=1)
        _oracle[key] = (img, tuple(int(getattr(st, f)) for f in COUNTERS))
    return _oracle[key]


def device(crt, desc):
    import torch
    scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], s["max_depth"], s["frame"], s["strategy"], s["filter"],
                                  s["filter_radius"], 0.0)
    r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
    r._protos = protos
    r.render_samples(0, rc.SPP)
    torch.cuda.synchronize()
    st = r.stats()
    scene.traversal_error()
    return r.image(), tuple(int(getattr(st, f)) for f in COUNTERS), r.pipeline(), r.lanes()


@pytest.mark.parametrize("pipeline", list(PIPELINES))
@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_the_oracle_and_the_closed_form(crt, monkeypatch, name, pipeline):
    case = CASES[name]
    env, fused, lanes = PIPELINES[pipeline]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    truth = case.truth()
    for s in case.strategies:
        means = []
        for frame in range(FRAMES):
            img, counters, pipe, ran_lanes = device(crt, case.build(s, frame))
            want_img, want_counters = oracle(case, s, frame)
            assert counters == want_counters, (name, s, frame, dict(zip(COUNTERS, zip(counters, want_counters))))
            bad = np.argwhere(img.view(np.uint32) != want_img.view(np.uint32))
            assert bad.shape[0] == 0, (name, s, frame, bad.shape[0], bad[:3])
            # no fused instance carries the lights at infinity (launch_plan.h, launch plan): of these scenes the fused
            # kernel takes the emissive interiors, asked for or by default, and every scene with a dome runs per stage
            at_infinity = any(l["kind"] in ("dome", "distant") for l in case.build(s, frame).lights)
            if fused is not None:
                assert pipe["fused"] is (fused and not at_infinity), (name, pipeline, pipe)
            elif at_infinity:
                assert pipe["fused"] is False, (name, pipeline, pipe)
            assert lanes is None or ran_lanes == lanes, (name, pipeline, ran_lanes)
            assert counters[COUNTERS.index("camera_rays")] == rc.W * rc.H * rc.SPP
            means.append(np.asarray(img, np.float64).mean(axis=(0, 1)))
        mean, se = rc.mean_and_se(np.array(means))
        print("%s %s %s: mean %.7f truth %.7f rel %+.2e, 5 SE %.2e" % (name, pipeline, s, mean[0], truth[0],
                                                                      mean[0] / truth[0] - 1.0, 5.0 * se[0] / truth[0]))
        assert np.all(np.abs(mean - truth) <= 5.0 * se + case.allowance(s) * truth), (name, s, mean, truth, se)
