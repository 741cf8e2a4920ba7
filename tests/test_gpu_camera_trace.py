"""Camera rays traced where they are made (pathtrace.hip, k_camera; LaunchPlan::camera_trace): one launch generates, culls
and traces a batch's camera rays, one ray per lane, and the first extend (k_extend_deferred) only picks up the rays that
loop left — leaves with scalar entries, a stack deeper than its LDS part.

A camera ray's traversal is the pool engine's, step for step, or the pool engine's own (a deferred ray starts again from
the root), so NOTHING the renderer reports may move: the frame's bits and all eight RayStats counters are compared — the
default (or CRT_CAMERA_TRACE=1) against CRT_CAMERA_TRACE=0, which runs the launches of before, and against the oracle's
integrator — with and without the root cull, through the pipelined and the plain shade kernel, with every ray deferred
(CRT_CAMERA_TRACE=2: the list and the deferred instance alone), with a one-entry stack (3: rays defer mid-tree), on the
packet-case scenes, on scenes the plan must keep out (instances with shading normals, a moving instance, lights, a lens),
on frames where every ray or no ray is culled, at depth 0 and 1, and on batches whose segments hold more slots than paths."""
import numpy as np
import pytest

import fuzz_scenes
import ora
import ora_world
import packet_cases as pc
from test_gpu_root_cull import COUNTERS, centre_rays_touched, scene_desc, gpu_render

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 4
_ORACLE = {}


def oracle(crt, key, desc, depth, spp, world=None):
    """The oracle's frame and counters: computed once per case, shared by the runs compared with it."""
    if key not in _ORACLE:
        oimg, ost = ora_world.OracleRenderer(desc, world or crt.usda, max_depth=depth).render(spp, forward=1)
        _ORACLE[key] = (oimg, tuple(int(getattr(ost, f)) for f in COUNTERS))
    return _ORACLE[key]


def render(crt, monkeypatch, desc, depth, spp, env, world=None):
    if world is None:
        with monkeypatch.context() as m:
            m.delenv("CRT_CAMERA_TRACE", raising=False)
            return gpu_render(crt, monkeypatch, desc, depth, spp, env)
    import torch
    with monkeypatch.context() as m:
        for k in ("CRT_CAMERA_TRACE", "CRT_ROOT_CULL", "CRT_LANES", "CRT_SHADE_PIPE", "CRT_CAM_COMPACT", "CRT_WIDE", "CRT_FUSED", "CRT_LANE_MIN_PATHS"):
            m.delenv(k, raising=False)
        for k, v in dict(dict(CRT_FUSED="0", CRT_LANE_MIN_PATHS="1"), **env).items():
            m.setenv(k, v)
        scene, mats, protos = world.build_world(desc, crt, crt.default_material)
        s = desc.settings
        settings = crt.RenderSettings(s["width"], s["height"], s["max_depth"] if depth is None else depth, s["frame"], s["strategy"],
                                      s["filter"], s["filter_radius"], 0.0)
        r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
        r._protos = protos
        r.render_samples(0, spp)
        torch.cuda.synchronize()
        st = r.stats()
        return r.image(), tuple(int(getattr(st, f)) for f in COUNTERS), r.pipeline(), r.lanes(), r


def both_ways(crt, monkeypatch, key, desc, depth, spp, env=None, knob=None, expect=True, world=None):
    """`knob` (None: unset, the host rule) | CRT_CAMERA_TRACE=0 | the oracle: same bits, same eight counters.
    -> (counters by name, the first run)"""
    env = dict(env or {})
    on = render(crt, monkeypatch, desc, depth, spp, dict(env, **({} if knob is None else dict(CRT_CAMERA_TRACE=knob))), world)
    off = render(crt, monkeypatch, desc, depth, spp, dict(env, CRT_CAMERA_TRACE="0"), world)
    assert on[2]["fused"] is False and off[2]["fused"] is False
    assert on[2]["camera_trace"] is expect and off[2]["camera_trace"] is False, (on[2], off[2])
    for k in ("wide", "shade_pipe", "root_cull", "slim_state", "grid"):
        assert on[2][k] == off[2][k], (k, on[2], off[2])  # the knob moves nothing else
    oimg, want = oracle(crt, key, desc, depth, spp, world)
    for tag, got in (("camera trace", on), ("CRT_CAMERA_TRACE=0", off)):
        assert got[1] == want, (tag, dict(zip(COUNTERS, zip(got[1], want))))
        bad = np.argwhere(got[0].view(np.uint32) != oimg.view(np.uint32))
        assert bad.shape[0] == 0, (tag, bad.shape[0], bad[:3])
    on[4].scene.traversal_error()
    return dict(zip(COUNTERS, want)), on


@pytest.mark.parametrize("env,knob,cull,pipe", [
    (dict(CRT_WIDE="1"), None, True, True),                           # the default: four lanes, root cull, pipelined shade
    (dict(CRT_WIDE="1", CRT_LANES="1"), None, True, True),            # one lane
    (dict(CRT_WIDE="1", CRT_ROOT_CULL="0"), None, False, True),       # every sample goes on and keeps its slot (plane a alone)
    (dict(CRT_WIDE="1", CRT_SHADE_PIPE="0"), None, True, False),      # the hit records read by the plain four-wave shade kernel
    (dict(CRT_WIDE="1"), "2", True, True),                            # every surviving ray deferred: the list, the deferred instance
    (dict(CRT_WIDE="1", CRT_ROOT_CULL="0"), "2", False, True),
    (dict(CRT_WIDE="1"), "3", True, True),                            # a one-entry stack: rays defer mid-tree
], ids=["default", "one-lane", "no-cull", "plain-shade", "defer-all", "defer-all-no-cull", "stack-1"])
def test_cornellbox(crt, monkeypatch, env, knob, cull, pipe):
    desc = scene_desc(crt, "cornellbox", W, H)
    st, on = both_ways(crt, monkeypatch, "cornellbox32", desc, 32, SPP, env, knob)
    assert on[2]["root_cull"] is cull and on[2]["shade_pipe"] is pipe and on[3] == (1 if env.get("CRT_LANES") == "1" else 4), on[2]
    assert st["camera_rays"] == W * H * SPP and 0.3 * st["camera_rays"] < st["ended_escaped"] and st["vertices"] > st["camera_rays"] // 2


@pytest.mark.parametrize("name", pc.NAMES)
def test_packet_case_scenes_without_their_light(crt, monkeypatch, name):
    """Mixed masks in one packet (camera rays carry CRT_MASK_CAMERA), several hits in one packet, the tie, the sliver — with
    the light list emptied so that the compact camera form applies (the emissive quad stays, as geometry). `normals` holds
    shading normals and a nested instance: the plan keeps it on the launches of before."""
    desc = pc.desc(crt.usda, name)
    desc.lights = []
    world = pc.World(crt.usda)
    st, on = both_ways(crt, monkeypatch, "pc-" + name, desc, None, SPP, dict(CRT_WIDE="1"), "1", expect=name != "normals", world=world)
    assert st["camera_rays"] == 64 * 36 * SPP and st["closest_hit"] > st["camera_rays"]


def test_tri_spheres(crt, monkeypatch):
    """The tessellated spheres of the traversal benchmarks (tests/scenes.py, tri_spheres) as an unlit world: a larger tree
    than the staged window holds, so nodes and packets come from both arms; asked for with the knob (the host rule keeps
    trees above kCameraTraceMaxNodes nodes out)."""
    import fixtures as fx
    desc = crt.usda.SceneDesc()
    for k, (v, i) in enumerate(fx.tri_spheres()):
        desc.geoms.append(pc._mesh(v, i, (0.3 + 0.1 * (k % 5), 0.6, 0.8 - 0.1 * (k % 4)), name="sphere %d" % k))
    desc.camera = dict(lookfrom=np.array([1.0, 2.0, 9.0], np.float32), lookat=np.array([0.0, 0.0, 0.0], np.float32),
                       vup=np.array([0, 1, 0], np.float32), vfov_deg=np.float32(50), aspect=np.float32(64 / 36), aperture=np.float32(0),
                       focus_dist=np.float32(6))
    desc.settings.update(width=64, height=36, max_depth=4, spp=4)
    st, on = both_ways(crt, monkeypatch, "tri_spheres", desc, None, SPP, dict(CRT_WIDE="1"), "1", world=pc.World(crt.usda))
    assert st["closest_hit"] > st["camera_rays"] and st["ended_escaped"] > 0


def test_a_lit_scene_keeps_the_launches_of_before(crt, monkeypatch):
    """veach_mis is lit: the plan keeps it out whatever the knob says."""
    desc = scene_desc(crt, "veach_mis", W, H)
    both_ways(crt, monkeypatch, "veach8", desc, 8, SPP, {}, "1", expect=False)


def test_an_instanced_world_with_a_moving_instance(crt, monkeypatch):
    """Fuzz world 114: instances, one moving, a rect light, general materials — the plan falls back, nothing differs."""
    desc = fuzz_scenes.random_world(crt.usda, 114, W, H)
    both_ways(crt, monkeypatch, "fuzz114", desc, None, SPP, {}, "1", expect=False)


def test_an_instanced_world_unlit(crt, monkeypatch):
    """... and the same world without its lights and its motion, on the four-wave kernels where they take it: camera rays
    that reach an instance defer. The plan may still keep it out (cold state); either way nothing differs."""
    desc = fuzz_scenes.random_world(crt.usda, 114, W, H)
    desc.lights = []
    for g in desc.geoms:
        g.pop("l2w_end", None)
    on = render(crt, monkeypatch, desc, None, SPP, dict(CRT_CAMERA_TRACE="1"))
    off = render(crt, monkeypatch, desc, None, SPP, dict(CRT_CAMERA_TRACE="0"))
    assert off[2]["camera_trace"] is False and on[1] == off[1]
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))


def test_a_camera_inside_the_bounds(crt, monkeypatch):
    cam = dict(lookfrom=np.array([0.0, 2.0, 1.5], np.float32), lookat=np.array([0.0, 2.0, -1.0], np.float32), vfov_deg=np.float32(60.0))
    desc = scene_desc(crt, "cornellbox", W, H, cam)
    st, on = both_ways(crt, monkeypatch, "inside6", desc, 6, SPP, dict(CRT_WIDE="1", CRT_ROOT_CULL="1"))
    assert centre_rays_touched(crt, desc, on[4].scene).all() and on[2]["root_cull"] is True


def test_a_camera_looking_away(crt, monkeypatch):
    """Every camera ray is finished by the cull: the first extend sees an empty list, the first shade empty segments."""
    desc = scene_desc(crt, "cornellbox", W, H, dict(lookat=np.array([0.0, 2.0, 9.0], np.float32)))
    st, on = both_ways(crt, monkeypatch, "away6", desc, 6, SPP, dict(CRT_WIDE="1"))
    assert st["closest_hit"] == st["ended_escaped"] == st["camera_rays"] == W * H * SPP and st["vertices"] == 0


@pytest.mark.parametrize("depth,expect", [(0, False), (1, True)])
def test_depth_limits_0_and_1(crt, monkeypatch, depth, expect):
    """max_depth 0: no first extend's result is ever used beyond ending the path; the plan keeps the launches of before."""
    desc = scene_desc(crt, "cornellbox", W, H)
    st, _on = both_ways(crt, monkeypatch, "depth%d" % depth, desc, depth, SPP, dict(CRT_WIDE="1"), expect=expect)
    assert st["ended_depth"] > 0


@pytest.mark.parametrize("w,h,spp", [(16, 16, 3), (37, 23, 1)], ids=["16x16x3", "37x23x1"])
@pytest.mark.parametrize("knob", ["1", "2"])
def test_segments_with_more_slots_than_paths(crt, monkeypatch, w, h, spp, knob):
    """768 paths (and 851, no multiple of the workgroup's width) dealt to 2 048 segments: the ragged end of the slot loop
    and of the list of deferred rays."""
    desc = scene_desc(crt, "cornellbox", w, h)
    st, on = both_ways(crt, monkeypatch, "ragged-%d-%d-%d" % (w, h, spp), desc, 6, spp, dict(CRT_WIDE="1", CRT_ROOT_CULL="1"), knob)
    assert on[2]["grid"] * 256 > 2 * w * h * spp and st["ended_escaped"] > 0


def test_the_default(crt, monkeypatch):
    """Unset, the host rule decides: on for cornellbox, off for veach_mis (lit) and for a lens camera."""
    for desc, want in ((scene_desc(crt, "cornellbox", W, H), True), (scene_desc(crt, "veach_mis", W, H), False),
                       (scene_desc(crt, "cornellbox", W, H, dict(aperture=np.float32(0.25), focus_dist=np.float32(4.0))), False)):
        got = render(crt, monkeypatch, desc, 4, 1, {})
        assert got[2]["camera_trace"] is want, (desc.camera, got[2])
