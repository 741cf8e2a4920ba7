"""The scenes of tests/image_cases.py on the device: 24 x 20 (and 260 x 2) at 256 spp, frames 0..3, through the default
pipeline, the fused kernel, one launch per stage, one lane, and — per stage, where the camera launches live — the
per-pixel table on and off, without k_camera, without k_camera_vertex, the root cull forced with its root in LDS and in
registers, without the root cull, and camera paths as full records. r.pipeline() says which form ran: a knob that did not
take tests nothing. The image bits and all eight RayStats equal the oracle's, and the closed-form bound of
tests/test_image_formation.py holds on the device's own image, in every pixel, row and column.

The stopping rule: every sample's colour read back one batch of one sample at a time, the adaptive counts against
image_ref.stop_count of those sequences, the image against the float32 sum of the samples taken, and the same render in
ragged batches (tests/test_gpu_render.py, test_adaptive_stopping_identical_to_oracle, holds batch independence on a lit
scene against the oracle; here it is held against the closed form)."""
import numpy as np
import pytest

import image_cases as ic
import ora

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in ic.cases()}
COUNTERS = [f for f, _t in ora.RayStats._fields_]
KNOBS = ("CRT_FUSED", "CRT_STAGE_MIN_PATHS", "CRT_PREFER_STAGE", "CRT_LANES", "CRT_LANE_MIN_PATHS", "CRT_WIDE", "CRT_SHADE_PIPE",
         "CRT_ROOT_CULL", "CRT_CAM_COMPACT", "CRT_GRID_MULT", "CRT_CAMERA_TRACE", "CRT_CAMERA_VERTEX", "CRT_PIXEL_TABLE",
         "CRT_SLIM_STATE", "CRT_CULL_ROOT_LDS")
STAGE = {"CRT_FUSED": "0"}
# name: (environment, what r.pipeline() must report — for every case / for the pinhole cases only —, lanes or None)
PIPELINES = {
    "default": ({}, dict(fused=True), {}, None),
    "fused": ({"CRT_FUSED": "1"}, dict(fused=True, camera_trace=False), {}, None),
    "per_stage": (STAGE, dict(fused=False), dict(camera_trace=True), None),
    "one_lane": ({"CRT_LANES": "1", "CRT_LANE_MIN_PATHS": "1"}, {}, {}, 1),
    "table_off": (dict(STAGE, CRT_PIXEL_TABLE="0"), dict(fused=False, pixel_table=False), dict(camera_trace=True), None),
    "table_on": (dict(STAGE, CRT_PIXEL_TABLE="1"), dict(fused=False), dict(camera_trace=True, pixel_table=True), None),
    "no_camera_trace": (dict(STAGE, CRT_CAMERA_TRACE="0"), dict(fused=False, camera_trace=False, camera_vertex=False, pixel_table=False), {}, None),
    "no_camera_vertex": (dict(STAGE, CRT_CAMERA_VERTEX="0"), dict(fused=False, camera_vertex=False), dict(camera_trace=True), None),
    "cull_root_lds": (dict(STAGE, CRT_ROOT_CULL="1"), dict(fused=False), dict(camera_trace=True, root_cull=True, cull_root_lds=True), None),
    "cull_root_registers": (dict(STAGE, CRT_ROOT_CULL="1", CRT_CULL_ROOT_LDS="0"), dict(fused=False, cull_root_lds=False),
                            dict(camera_trace=True, root_cull=True), None),
    "no_root_cull": (dict(STAGE, CRT_ROOT_CULL="0"), dict(fused=False, root_cull=False, cull_root_lds=False), dict(camera_trace=True), None),
    "full_records": (dict(STAGE, CRT_CAM_COMPACT="0"), dict(fused=False, camera_trace=False), {}, None),
}
_oracle, _oracle_samples = {}, {}


def oracle(case, frame):
    """The oracle's image and counters of one frame, rendered once for all the pipelines."""
    key = (case.name, frame)
    if key not in _oracle:
        import ora_world
        img, st = ora_world.OracleRenderer(case.build(frame), ic.usda).render(ic.SPP, forward=1)
        _oracle[key] = (img, tuple(int(getattr(st, f)) for f in COUNTERS))
    return _oracle[key]


def renderer(crt, desc, variance=0.0, min_spp=None):
    scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], s["max_depth"], s["frame"], s["strategy"], s["filter"],
                                  s["filter_radius"], variance, s["min_spp"] if min_spp is None else min_spp)
    r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
    r._protos = protos
    return r


def device(crt, desc):
    import torch
    r = renderer(crt, desc)
    r.render_samples(0, ic.SPP)
    torch.cuda.synchronize()
    st = r.stats()
    r.scene.traversal_error()
    return r.image(), tuple(int(getattr(st, f)) for f in COUNTERS), r.pipeline(), r.lanes()


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("pipeline", list(PIPELINES))
@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_the_oracle_and_the_closed_form(crt, monkeypatch, name, pipeline):
    case = CASES[name]
    env, always, pinhole, lanes = PIPELINES[pipeline]
    set_knobs(monkeypatch, env)
    images = []
    for frame in range(ic.FRAMES):
        img, counters, pipe, ran_lanes = device(crt, case.build(frame))
        want_img, want_counters = oracle(case, frame)
        assert counters == want_counters, (name, frame, dict(zip(COUNTERS, zip(counters, want_counters))))
        bad = np.argwhere(img.view(np.uint32) != want_img.view(np.uint32))
        assert bad.shape[0] == 0, (name, frame, bad.shape[0], bad[:3])
        assert counters[COUNTERS.index("camera_rays")] == case.width * case.height * ic.SPP
        want_pipe = dict(always, **(pinhole if case.pinhole else {}))
        if not case.pinhole:  # a lens and a moving instance both keep the camera launches and the compact records out
            want_pipe.update(camera_trace=False, camera_vertex=False, pixel_table=False)
        assert {k: pipe[k] for k in want_pipe} == want_pipe, (name, pipeline, pipe)
        assert lanes is None or ran_lanes == lanes, (name, pipeline, ran_lanes)
        images.append(np.asarray(img, np.float64))
    mean = np.mean(images, axis=0)
    bad = ic.violations(case, mean, ic.FRAMES * ic.SPP, case.allowance())
    print("%s %s: largest deviation %.2e of the contrast, %d violations, %s" % (name, pipeline, ic.deviation(case, mean), len(bad), pipe))
    assert not bad, (name, pipeline, len(bad), bad[:4])
    if case.half_plane is None:
        assert all(np.all(i == ic.BACKDROP) for i in images)


def test_the_pinhole_cases_reach_both_camera_launches(crt, monkeypatch):
    """Per stage and left to itself, the slanted case runs k_camera_vertex with the per-pixel table; CRT_CAMERA_VERTEX=0
    leaves k_camera with the table: both camera launches and both forms of camera_sample are among the pipelines above."""
    case = CASES["pinhole_slanted"]
    set_knobs(monkeypatch, STAGE)
    pipe = device(crt, case.build(0))[2]
    assert pipe["camera_trace"] and pipe["camera_vertex"] and pipe["pixel_table"], pipe
    set_knobs(monkeypatch, dict(STAGE, CRT_CAMERA_VERTEX="0"))
    pipe = device(crt, case.build(0))[2]
    assert pipe["camera_trace"] and not pipe["camera_vertex"] and pipe["pixel_table"], pipe


# ---------------------------------------------------------------- the stopping rule ----------------------------------------------------------------
def device_samples(crt, case):
    """[height, width, 64, 3]: the film after one batch of one sample, cleared between them."""
    import torch
    r = renderer(crt, case.build(0))
    out = np.zeros((case.height, case.width, ic.STOP_SPP, 3), np.float32)
    for s in range(ic.STOP_SPP):
        r.render_samples(s, 1)
        torch.cuda.synchronize()
        out[:, :, s] = r.image()
        r.clear()
    return out


def counts_image(r, case):
    out = np.zeros(case.height * case.width, np.uint32)
    out[r.pixel_indices()] = r.sample_counts()
    return out.reshape(case.height, case.width)


@pytest.mark.parametrize("pipeline", ["default", "per_stage"])
@pytest.mark.parametrize("luminance", [None, 3e-5], ids=["bright", "under-the-floor"])
def test_device_stops_where_the_rule_says(crt, monkeypatch, luminance, pipeline):
    import torch
    set_knobs(monkeypatch, PIPELINES[pipeline][0])
    case = ic.stop_case(luminance)
    samples = device_samples(crt, case)
    if luminance not in _oracle_samples:
        _oracle_samples[luminance] = ic.oracle_samples(case, ic.STOP_SPP)
    assert np.array_equal(samples.view(np.uint32), _oracle_samples[luminance].view(np.uint32))
    for min_spp, threshold in ic.STOP_RULES:
        want, lit = ic.expected_counts(case, samples, min_spp, threshold)  # asserts the samples are two-valued
        r = renderer(crt, case.build(0), threshold, min_spp)
        r.render_adaptive(ic.STOP_SPP)
        torch.cuda.synchronize()
        counts, img, st = counts_image(r, case), r.image(), r.stats()
        assert np.array_equal(counts, want), (min_spp, threshold, np.argwhere(counts != want)[:4], counts[counts != want][:4], want[counts != want][:4])
        ic.check_stop_shape(counts, lit, min_spp, threshold, bright=luminance is None)
        assert np.array_equal(img.view(np.uint32), ic.sequential_mean(samples, counts).view(np.uint32)), (min_spp, threshold)
        assert st.camera_rays == int(counts.sum())  # batches of 4 after the first look: no sample traced in vain
        o_counts, o_img = ic.oracle_adaptive(case, ic.STOP_SPP, min_spp, threshold)
        assert np.array_equal(counts, o_counts) and np.array_equal(img.view(np.uint32), o_img.view(np.uint32))
        # the same render in ragged batches (crt.h, CrtRenderSettings: the rule is evaluated sample by sample in the fold)
        r2 = renderer(crt, case.build(0), threshold, min_spp)
        for begin, n in ((0, 3), (3, 1), (4, 4), (8, 7), (15, 49)):
            r2.render_samples(begin, n)
        torch.cuda.synchronize()
        assert np.array_equal(counts_image(r2, case), counts), (min_spp, threshold)
        assert np.array_equal(r2.image().view(np.uint32), img.view(np.uint32)), (min_spp, threshold)
