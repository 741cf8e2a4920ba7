"""The root cull of the per-stage pipeline (pathtrace.hip, generate_segment_cull): camera rays that touch no child box of
the root node are finished in generate — sky gradient into the staging film, closest_hit and ended_escaped counted — and
only the others are appended to the segments.

The ray is still traced, its traversal being the root step, so NOTHING the renderer reports may move: the frame's bits and
all eight RayStats counters are compared three ways — the default against CRT_ROOT_CULL=0, against the oracle's
integrator, and again as one lane (CRT_LANES=1) — on every form of camera path the cull touches: the 16-byte compact form
with its plane d read back by the pipelined and by the plain shade kernel, the full form of lit scenes with shadow rays,
lens cameras, moving instances, adaptive stopping, frames where nothing or everything is culled, depth limits 0 and 1,
and batches whose segments hold more slots than paths.

By default the renderer culls only where its estimate of the frame's background share says it pays (an eighth of a coarse
grid of camera rays miss the root's boxes: cornellbox 0.44, veach_mis 0.06). The cases whose frame shows less are run with
CRT_ROOT_CULL=1, which skips the estimate, so the cull's code runs on them all the same."""
import ctypes as C
import os

import numpy as np
import pytest

import fuzz_scenes
import ora
import ora_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

COUNTERS = [f for f, _t in ora.RayStats._fields_]
# the per-stage pipeline whatever the batch size; lanes split down to one sample each
BASE = dict(CRT_FUSED="0", CRT_LANE_MIN_PATHS="1")
KNOBS = ("CRT_ROOT_CULL", "CRT_LANES", "CRT_SHADE_PIPE", "CRT_CAM_COMPACT", "CRT_WIDE", "CRT_FUSED", "CRT_LANE_MIN_PATHS",
         "CRT_GRID_MULT")


def scene_desc(crt, name, w, h, camera=None):
    desc = crt.usda.load(os.path.join(ROOT, "scenes", name + ".usda"), w, h)
    if camera:
        desc.camera = dict(desc.camera, **camera)
    return desc


def gpu_render(crt, monkeypatch, desc, depth, spp, env, variance=0.0, min_spp=None):
    """One render with the knobs of `env` (read when the renderer is made) -> image, counters, pipeline, lanes."""
    import torch
    with monkeypatch.context() as m:
        for k in KNOBS:
            m.delenv(k, raising=False)
        for k, v in dict(BASE, **env).items():
            m.setenv(k, v)
        scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
        s = desc.settings
        settings = crt.RenderSettings(s["width"], s["height"], s["max_depth"] if depth is None else depth, s["frame"], s["strategy"],
                                      s["filter"], s["filter_radius"], float(variance), s["min_spp"] if min_spp is None else min_spp)
        r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
        r._protos = protos
        if variance > 0.0:
            r.render_adaptive(spp)
        else:
            r.render_samples(0, spp)
        torch.cuda.synchronize()
        st = r.stats()
        return r.image(), tuple(int(getattr(st, f)) for f in COUNTERS), r.pipeline(), r.lanes(), r


def three_ways(crt, monkeypatch, desc, depth, spp, env=None, variance=0.0, min_spp=None, expect_cull=True, lanes=4, force=False):
    """default (force: CRT_ROOT_CULL=1) | CRT_ROOT_CULL=0 | one lane | the oracle: same bits, same eight counters.
    -> (counters, the first renderer)"""
    env = dict(env or {}, **(dict(CRT_ROOT_CULL="1") if force else {}))
    on = gpu_render(crt, monkeypatch, desc, depth, spp, env, variance, min_spp)
    off = gpu_render(crt, monkeypatch, desc, depth, spp, dict(env, CRT_ROOT_CULL="0"), variance, min_spp)
    one = gpu_render(crt, monkeypatch, desc, depth, spp, dict(env, CRT_LANES="1"), variance, min_spp)
    assert on[2]["fused"] is False and off[2]["fused"] is False and one[2]["fused"] is False
    assert on[2]["root_cull"] is expect_cull and one[2]["root_cull"] is expect_cull and off[2]["root_cull"] is False, (on[2], off[2])
    assert on[3] == lanes and one[3] == 1, (on[3], one[3])
    o = ora_world.OracleRenderer(desc, crt.usda, max_depth=depth, variance=variance, min_spp=min_spp)
    oimg, ost = o.render(spp, forward=1)
    want = tuple(int(getattr(ost, f)) for f in COUNTERS)
    for tag, got in (("default", on), ("CRT_ROOT_CULL=0", off), ("CRT_LANES=1", one)):
        assert got[1] == want, (tag, dict(zip(COUNTERS, zip(got[1], want))))
        bad = np.argwhere(got[0].view(np.uint32) != oimg.view(np.uint32))
        assert bad.shape[0] == 0, (tag, bad.shape[0], bad[:3])
    return dict(zip(COUNTERS, want)), on


def centre_rays_touched(crt, desc, scene):
    """The root step of the frame's pixel-centre camera rays, on the host (crt_scene_root_touched_n)."""
    w, h = desc.settings["width"], desc.settings["height"]
    o = ora_world.OracleRenderer(desc, crt.usda)
    rays = np.zeros((w * h, 6), np.float32)
    for k in range(w * h):
        r = ora.Ray()
        ora.lib().ora_camera_get_ray(C.byref(o.job.camera), (k % w + 0.5) / w, (k // w + 0.5) / h, 0.5, 0.5, 0.0, C.byref(r))
        rays[k, 0:3] = r.origin.np()
        rays[k, 3:6] = r.dir.np()
    return scene.root_touched(rays)[0]


W, H, SPP = 64, 36, 4


@pytest.mark.parametrize("env,pipe,depth", [
    (dict(CRT_WIDE="1"), True, 32),                          # compact form + plane d, the pipelined shade kernel
    (dict(CRT_WIDE="1", CRT_SHADE_PIPE="0"), False, 32),     # ... read back by the plain four-wave kernel
    (dict(CRT_WIDE="0"), False, 8),                          # ... and by the three-wave kernel
    (dict(CRT_WIDE="1", CRT_CAM_COMPACT="0"), True, 8),      # the full form in an unlit scene
], ids=["pipe", "plain", "three-wave", "full-form"])
def test_cornellbox(crt, monkeypatch, env, pipe, depth):
    desc = scene_desc(crt, "cornellbox", W, H)
    st, on = three_ways(crt, monkeypatch, desc, depth, SPP, env)
    assert on[2]["shade_pipe"] is pipe, on[2]
    # the cull had rays to finish: by the host build of its predicate, well over a third of this frame's camera rays miss
    # every child box of the root (a cull that kept every ray would pass the comparisons above all the same)
    assert float(np.mean(~centre_rays_touched(crt, desc, on[4].scene))) > 0.35
    # an open frame: a good part of the camera rays escape, and paths that bounce escape later too
    assert st["camera_rays"] == W * H * SPP and 0.3 * st["camera_rays"] < st["ended_escaped"] and st["vertices"] > st["camera_rays"] // 2


def test_veach_mis_lit_full_form_with_shadow_rays(crt, monkeypatch):
    desc = scene_desc(crt, "veach_mis", W, H)
    st, on = three_ways(crt, monkeypatch, desc, 8, SPP, force=True)
    assert st["shadow_rays"] > 0 and st["ended_escaped"] > 0 and on[2]["shade_pipe"] is False


def test_a_camera_inside_the_bounds_culls_nothing(crt, monkeypatch):
    cam = dict(lookfrom=np.array([0.0, 2.0, 1.5], np.float32), lookat=np.array([0.0, 2.0, -1.0], np.float32), vfov_deg=np.float32(60.0))
    desc = scene_desc(crt, "cornellbox", W, H, cam)
    st, on = three_ways(crt, monkeypatch, desc, 6, SPP, dict(CRT_WIDE="1"), force=True)
    assert centre_rays_touched(crt, desc, on[4].scene).all()


def test_a_camera_looking_away_culls_every_ray(crt, monkeypatch):
    """Every camera ray is finished in generate: the first extend and the first shade see empty segments."""
    cam = dict(lookat=np.array([0.0, 2.0, 9.0], np.float32))
    desc = scene_desc(crt, "cornellbox", W, H, cam)
    st, on = three_ways(crt, monkeypatch, desc, 6, SPP, dict(CRT_WIDE="1"))
    assert not centre_rays_touched(crt, desc, on[4].scene).any()
    assert st["closest_hit"] == st["ended_escaped"] == st["camera_rays"] == W * H * SPP and st["vertices"] == 0


def test_a_lens_camera(crt, monkeypatch):
    """Per-ray origins: the full form in an unlit scene, the root step from the lens sample."""
    desc = scene_desc(crt, "cornellbox", W, H, dict(aperture=np.float32(0.25), focus_dist=np.float32(4.0)))
    st, _on = three_ways(crt, monkeypatch, desc, 6, SPP, dict(CRT_WIDE="1"))
    assert st["ended_escaped"] > 0


def test_an_instanced_world_with_a_moving_instance(crt, monkeypatch):
    """Fuzz world 114: six placements of a prototype under the top-level tree, one of them moving (shutter times: the time
    plane of the full form), a rect light, general materials — no light at infinity, so the cull is on."""
    desc = fuzz_scenes.random_world(crt.usda, 114, W, H)
    assert sum(g["kind"] == "instance" for g in desc.geoms) >= 2 and any("l2w_end" in g for g in desc.geoms)
    assert not [l for l in desc.lights if l["kind"] in ("distant", "dome")]
    st, _on = three_ways(crt, monkeypatch, desc, None, SPP, force=True)
    assert st["ended_escaped"] > 0 and st["shadow_rays"] > 0


def test_adaptive_stopping(crt, monkeypatch):
    """A threshold that stops some pixels after the first batch: later batches run over the active list (Params::active),
    and a culled sample lands in its ACTIVE slot of the staging film."""
    desc = scene_desc(crt, "veach_mis", W, H)
    st, on = three_ways(crt, monkeypatch, desc, 8, 48, variance=0.08, min_spp=8, lanes=1, force=True)
    counts = on[4].sample_counts()
    assert 0 < (counts < 48).sum() < counts.size, "the threshold should stop some pixels early and not others"
    assert st["camera_rays"] == int(counts.sum())


@pytest.mark.parametrize("depth,cull", [(0, False), (1, True)])
def test_depth_limits_0_and_1(crt, monkeypatch, depth, cull):
    """max_depth 0: an escaping path adds nothing (no depth left), so the host keeps the cull off; 1: on."""
    desc = scene_desc(crt, "cornellbox", W, H)
    st, _on = three_ways(crt, monkeypatch, desc, depth, SPP, dict(CRT_WIDE="1"), expect_cull=cull)
    assert st["ended_depth"] > 0
    if depth == 0:
        assert st["ended_escaped"] == 0


@pytest.mark.parametrize("w,h,spp", [(16, 16, 3), (37, 23, 1)], ids=["16x16x3", "37x23x1"])
def test_segments_with_more_slots_than_paths(crt, monkeypatch, w, h, spp):
    """768 paths (and 851, no multiple of the workgroup's width) dealt to thousands of segments: most segments are empty,
    a few hold one round, one a partial round — the uniform slot loop's ragged end."""
    desc = scene_desc(crt, "cornellbox", w, h)
    # (forced: a square frame of this camera shows too little background for the default to cull)
    st, on = three_ways(crt, monkeypatch, desc, 6, spp, dict(CRT_WIDE="1"), lanes=min(spp, 4), force=True)
    assert on[2]["grid"] * 256 > 2 * w * h * spp and st["ended_escaped"] > 0


def test_the_default_follows_the_share_of_the_frame_that_shows_background(crt, monkeypatch):
    """Unset, the knob leaves the choice to the renderer's estimate (Renderer::estimate_root_miss_share): on for cornellbox
    (0.44 of the grid's rays miss the root's boxes) and for a camera that sees nothing, off for veach_mis (0.06) and for a
    camera inside the bounds — which then run exactly the launches they ran before the cull existed."""
    inside = dict(lookfrom=np.array([0.0, 2.0, 1.5], np.float32), lookat=np.array([0.0, 2.0, -1.0], np.float32), vfov_deg=np.float32(60.0))
    for desc, want in ((scene_desc(crt, "cornellbox", W, H), True), (scene_desc(crt, "veach_mis", W, H), False),
                       (scene_desc(crt, "cornellbox", W, H, inside), False),
                       (scene_desc(crt, "cornellbox", W, H, dict(lookat=np.array([0.0, 2.0, 9.0], np.float32))), True)):
        got = gpu_render(crt, monkeypatch, desc, 4, 1, {})
        assert got[2]["root_cull"] is want, (desc.camera, got[2])
        share = float(np.mean(~centre_rays_touched(crt, desc, got[4].scene)))
        assert (share >= 0.125) is want, share
