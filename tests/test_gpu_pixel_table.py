"""The per-pixel camera table (kernels/camera_pixel.hip.h; pathtrace.hip, camera_sample_table, k_fill_pixel_table;
LaunchPlan::pixel_table): behind either camera launch the sample loop loads what a sample owes to its pixel alone — the
coordinates, the K_CAMERA domain's five Owen seeds, the K_PATH domain's pattern — from a 32-byte record the renderer
filled at creation, and steps each lane's (pixel, sample) pair from round to round instead of dividing.

NOTHING the renderer reports may move: the frame's bits and all eight RayStats counters are compared — the default against
CRT_PIXEL_TABLE=0 (the computed form) and against the oracle's integrator. cornellbox at 96 x 54 (20.25 rounds of 256 per
sample plane: the cursor wraps mid-round) and 192 x 108, 12 spp, depth 0, 1 and 32, four lanes and one; an spp that is a
multiple of nothing; without the root cull; the full path state; behind k_camera instead of k_camera_vertex; every ray
deferred and a one-entry stack; an instanced scene; a camera inside the bounds and one looking away; two shards.

The same comparison for the cull's root read from the LDS window (LaunchPlan::cull_root_lds, the default) against
CRT_CULL_ROOT_LDS=0 (the root's words in registers) and the oracle."""
import numpy as np
import pytest

from test_gpu_camera_trace import oracle
from test_gpu_root_cull import BASE, COUNTERS, scene_desc

pytestmark = pytest.mark.gpu

SPP = 12
KNOBS = ("CRT_PIXEL_TABLE", "CRT_CULL_ROOT_LDS", "CRT_CAMERA_TRACE", "CRT_CAMERA_VERTEX", "CRT_ROOT_CULL", "CRT_LANES", "CRT_SHADE_PIPE", "CRT_CAM_COMPACT", "CRT_WIDE",
         "CRT_FUSED", "CRT_LANE_MIN_PATHS", "CRT_GRID_MULT", "CRT_SLIM_STATE", "CRT_TAIL_FROM", "CRT_NOCLASSIFY_FROM")


def render(crt, monkeypatch, desc, depth, spp, env, rank=0, world=1):
    """One render with the knobs of `env` (read when the renderer is made) -> film of the owned pixels, counters, pipeline,
    lanes, renderer."""
    import torch
    with monkeypatch.context() as m:
        for k in KNOBS:
            m.delenv(k, raising=False)
        for k, v in dict(BASE, **env).items():
            m.setenv(k, v)
        scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
        s = desc.settings
        settings = crt.RenderSettings(s["width"], s["height"], s["max_depth"] if depth is None else depth, s["frame"], s["strategy"],
                                      s["filter"], s["filter_radius"], 0.0, s["min_spp"])
        r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings, rank, world)
        r._protos = protos
        r.render_samples(0, spp)
        torch.cuda.synchronize()
        st = r.stats()
        return r.film(), tuple(int(getattr(st, f)) for f in COUNTERS), r.pipeline(), r.lanes(), r


def both_ways(crt, monkeypatch, key, desc, depth, spp, env=None, expect=True, vertex=True):
    """default | CRT_PIXEL_TABLE=0 | the oracle: same bits, same eight counters. -> (counters by name, the first run)"""
    env = dict(env or {})
    on = render(crt, monkeypatch, desc, depth, spp, env)
    off = render(crt, monkeypatch, desc, depth, spp, dict(env, CRT_PIXEL_TABLE="0"))
    assert on[2]["pixel_table"] is expect and off[2]["pixel_table"] is False, (on[2], off[2])
    assert on[2]["camera_trace"] is expect and on[2]["camera_vertex"] is (expect and vertex), on[2]
    for k in on[2]:
        if k != "pixel_table":
            assert on[2][k] == off[2][k], (k, on[2], off[2])  # the knob moves nothing else
    assert on[2]["fused"] is False and on[3] == off[3]
    oimg, want = oracle(crt, key, desc, depth, spp)
    ofilm = oimg.reshape(-1, 3)[on[4].pixel_indices()]
    for tag, got in (("pixel table", on), ("CRT_PIXEL_TABLE=0", off)):
        print(tag, dict(zip(COUNTERS, got[1])))
        assert got[1] == want, (tag, dict(zip(COUNTERS, zip(got[1], want))))
        bad = np.argwhere(got[0].view(np.uint32) != ofilm.view(np.uint32))
        assert bad.shape[0] == 0, (tag, bad.shape[0], bad[:3])
    on[4].scene.traversal_error()
    return dict(zip(COUNTERS, want)), on


@pytest.mark.parametrize("w,h", [(96, 54), (192, 108)], ids=["96x54", "192x108"])
@pytest.mark.parametrize("depth", [0, 1, 32])
@pytest.mark.parametrize("lanes", ["4", "1"])
def test_cornellbox(crt, monkeypatch, w, h, depth, lanes):
    desc = scene_desc(crt, "cornellbox", w, h)
    env = dict(CRT_WIDE="1", CRT_LANES=lanes)
    st, on = both_ways(crt, monkeypatch, "cornellbox%d-%d-12" % (depth, w), desc, depth, SPP, env, expect=depth >= 1)
    assert on[3] == int(lanes) and st["camera_rays"] == w * h * SPP
    if depth >= 1:
        assert on[2]["root_cull"] is True and 0.3 * st["camera_rays"] < st["ended_escaped"]


@pytest.mark.parametrize("env,vertex", [
    (dict(CRT_WIDE="1", CRT_ROOT_CULL="0"), True),       # every sample goes on: the trace finishes the misses
    (dict(CRT_WIDE="1", CRT_SLIM_STATE="0"), True),      # the survivors leave in the full four planes
    (dict(CRT_WIDE="1", CRT_CAMERA_VERTEX="0"), False),  # k_camera<TABLE>: planes a and d and the hit records for a first shade
    (dict(CRT_WIDE="1", CRT_CAMERA_VERTEX="0", CRT_ROOT_CULL="0"), False),  # ... where a sample keeps the slot it was dealt
    (dict(CRT_WIDE="1", CRT_CAMERA_TRACE="2"), True),    # every surviving ray deferred: plane d carries the cursor's pair
    (dict(CRT_WIDE="1", CRT_CAMERA_TRACE="3"), True),    # a one-entry stack: hits and deferred rays in one round
], ids=["no-cull", "full-state", "k-camera", "k-camera-no-cull", "defer-all", "stack-1"])
def test_cornellbox_forms(crt, monkeypatch, env, vertex):
    desc = scene_desc(crt, "cornellbox", 96, 54)
    st, on = both_ways(crt, monkeypatch, "cornellbox32-96-12", desc, 32, SPP, env, vertex=vertex)
    assert st["vertices"] > st["camera_rays"] // 2


@pytest.mark.parametrize("spp,lanes", [(7, "4"), (7, "1"), (1, "1")])
def test_ragged_segments(crt, monkeypatch, spp, lanes):
    """7 samples on four lanes: sub-batches of 2, 2, 2 and 1 samples; 5 184 x 7 paths on one: 141.75 rounds of 256, so the
    last round's lanes run past the end, and a segment's cursor wraps the pixel list at a different lane every sample."""
    desc = scene_desc(crt, "cornellbox", 96, 54)
    st, on = both_ways(crt, monkeypatch, "cornellbox6-96-%d" % spp, desc, 6, spp, dict(CRT_WIDE="1", CRT_LANES=lanes))
    assert (96 * 54 * spp) % 256 != 0 and st["camera_rays"] == 96 * 54 * spp


def test_a_small_grid_steps_the_cursor_many_rounds(crt, monkeypatch):
    """CRT_GRID_MULT=1: a grid of one workgroup per CU, so a lane takes several rounds and its cursor several steps."""
    desc = scene_desc(crt, "cornellbox", 192, 108)
    st, on = both_ways(crt, monkeypatch, "cornellbox1-192-12", desc, 1, SPP, dict(CRT_WIDE="1", CRT_LANES="1", CRT_GRID_MULT="1"))
    assert 192 * 108 * SPP > 2 * on[2]["grid"] * 256  # more than two rounds per lane


@pytest.mark.parametrize("name", ["instancing", "nested_instancing"])
def test_instanced_scenes(crt, monkeypatch, name):
    """Whatever the plan makes of them — a camera launch with its deferred rays, or the launches of before — the table
    follows the camera launch and the frame keeps its bits."""
    desc = scene_desc(crt, name, 64, 36)
    desc.lights = []
    plain = render(crt, monkeypatch, desc, 6, 4, dict(CRT_WIDE="1", CRT_CAMERA_TRACE="1", CRT_PIXEL_TABLE="0"))
    both_ways(crt, monkeypatch, name + "6-unlit", desc, 6, 4, dict(CRT_WIDE="1", CRT_CAMERA_TRACE="1"), expect=plain[2]["camera_trace"],
              vertex=plain[2]["camera_vertex"])


def test_a_camera_inside_the_bounds(crt, monkeypatch):
    cam = dict(lookfrom=np.array([0.0, 2.0, 1.5], np.float32), lookat=np.array([0.0, 2.0, -1.0], np.float32), vfov_deg=np.float32(60.0))
    desc = scene_desc(crt, "cornellbox", 64, 36, cam)
    st, on = both_ways(crt, monkeypatch, "inside6", desc, 6, 4, dict(CRT_WIDE="1", CRT_ROOT_CULL="1"))
    assert st["vertices"] >= st["camera_rays"]  # every camera ray hits


def test_a_camera_looking_away(crt, monkeypatch):
    desc = scene_desc(crt, "cornellbox", 64, 36, dict(lookat=np.array([0.0, 2.0, 9.0], np.float32)))
    st, on = both_ways(crt, monkeypatch, "away6", desc, 6, 4, dict(CRT_WIDE="1"))
    assert st["closest_hit"] == st["ended_escaped"] == st["camera_rays"] and st["vertices"] == 0


@pytest.mark.parametrize("env,vertex", [
    (dict(CRT_WIDE="1"), True),
    (dict(CRT_WIDE="1", CRT_LANES="1", CRT_PIXEL_TABLE="0"), True),
    (dict(CRT_WIDE="1", CRT_CAMERA_VERTEX="0"), False),
    (dict(CRT_WIDE="1", CRT_CAMERA_TRACE="3"), True),
], ids=["default", "one-lane-computed", "k-camera", "stack-1"])
def test_the_cull_reads_the_root_from_the_lds_window(crt, monkeypatch, env, vertex):
    """The cull's predicate on the staged root (the default; CRT_CULL_ROOT_LDS=0: the root's words in registers): the same
    frame, the same counters, against the registers' form and the oracle; without the root cull there is nothing to switch."""
    desc = scene_desc(crt, "cornellbox", 96, 54)
    oimg, want = oracle(crt, "cornellbox32-96-12", desc, 32, SPP)
    off = render(crt, monkeypatch, desc, 32, SPP, dict(env, CRT_CULL_ROOT_LDS="0"))
    on = render(crt, monkeypatch, desc, 32, SPP, env)
    none = render(crt, monkeypatch, desc, 32, SPP, dict(env, CRT_ROOT_CULL="0"))
    assert on[2]["cull_root_lds"] is True and off[2]["cull_root_lds"] is False and none[2]["cull_root_lds"] is False
    assert on[2]["camera_vertex"] is vertex and on[2]["root_cull"] is True
    for k in on[2]:
        if k != "cull_root_lds":
            assert on[2][k] == off[2][k], (k, on[2], off[2])  # the knob moves nothing else
    ofilm = oimg.reshape(-1, 3)[on[4].pixel_indices()]
    for tag, got in (("registers", off), ("lds", on), ("no cull", none)):
        assert got[1] == want, (tag, dict(zip(COUNTERS, zip(got[1], want))))
        assert np.array_equal(got[0].view(np.uint32), ofilm.view(np.uint32)), tag


def test_two_shards_index_the_table_by_their_own_pixel_slots(crt, monkeypatch):
    """80 x 48 = 5 x 3 tiles dealt to two ranks: 8 and 7 tiles. Each rank's film is the oracle's frame at its pixels."""
    desc = scene_desc(crt, "cornellbox", 80, 48)
    oimg, _st = oracle(crt, "cornellbox6-80", desc, 6, 4)
    seen = np.zeros(80 * 48, bool)
    for rank in range(2):
        on = render(crt, monkeypatch, desc, 6, 4, dict(CRT_WIDE="1"), rank, 2)
        off = render(crt, monkeypatch, desc, 6, 4, dict(CRT_WIDE="1", CRT_PIXEL_TABLE="0"), rank, 2)
        assert on[2]["pixel_table"] is True and off[2]["pixel_table"] is False
        idx = on[4].pixel_indices()
        assert len(idx) == (8, 7)[rank] * 256 and not seen[idx].any()
        seen[idx] = True
        assert on[1] == off[1]
        assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
        assert np.array_equal(on[0].view(np.uint32), oimg.reshape(-1, 3)[idx].view(np.uint32))
    assert seen.all()
