"""The first vertex shaded in the lane that traced the camera ray (pathtrace.hip, k_camera_vertex; vertex_simple.hip.h;
LaunchPlan::camera_vertex): behind camera_trace a hit runs the vertex function the pipelined shade kernel calls, with a
camera path's constants, and its survivor goes straight to the other state buffer; a miss ends on the sky; a deferred ray
goes to the input buffer, and the first extend and the first k_shade_pipe launch (append mode) see only those.

NOTHING the renderer reports may move: the frame's bits and all eight RayStats counters are compared — the default against
CRT_CAMERA_VERTEX=0 (k_camera and a first shade over every path), against CRT_CAMERA_TRACE=0 (generate and a first extend
over every ray) and against the oracle's integrator. Frames of 96 x 54 and 64 x 36 at 4 spp: 20 736 and 9 216 paths dealt
in rounds of 256, four lanes of one sample each — a segment's two lists hold what the cull, the misses and the split
between survivors and deferred rays leave of a round: ragged, not multiples of 256."""
import numpy as np
import pytest

import fixtures as fx
import packet_cases as pc
from test_camera_trace_host import MISS, HIT, DEFER, host, trace  # noqa: F401  (host: the module's fixture)
from test_gpu_camera_trace import oracle, render as render_trace
from test_gpu_root_cull import COUNTERS, scene_desc

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 54, 4
KNOBS = ("CRT_CAMERA_VERTEX", "CRT_TAIL_FROM", "CRT_NOCLASSIFY_FROM", "CRT_SLIM_STATE")


def render(crt, monkeypatch, desc, depth, spp, env, world=None):
    with monkeypatch.context() as m:
        for k in KNOBS:
            m.delenv(k, raising=False)
        for k in KNOBS:
            if k in env:
                m.setenv(k, env[k])
        rest = {k: v for k, v in env.items() if k not in KNOBS}
        return render_trace(crt, monkeypatch, desc, depth, spp, rest, world)


def three_ways(crt, monkeypatch, key, desc, depth, spp, env=None, expect=True, world=None, trace_on=True):
    """default | CRT_CAMERA_VERTEX=0 | CRT_CAMERA_TRACE=0 | the oracle: same bits, same eight counters.
    -> (counters by name, the first run)"""
    env = dict(env or {})
    on = render(crt, monkeypatch, desc, depth, spp, env, world)
    off = render(crt, monkeypatch, desc, depth, spp, dict(env, CRT_CAMERA_VERTEX="0"), world)
    plain = render(crt, monkeypatch, desc, depth, spp, dict(env, CRT_CAMERA_TRACE="0"), world)
    assert on[2]["camera_vertex"] is expect and off[2]["camera_vertex"] is False and plain[2]["camera_vertex"] is False, (on[2], off[2], plain[2])
    assert on[2]["camera_trace"] is trace_on and off[2]["camera_trace"] is trace_on and plain[2]["camera_trace"] is False
    for k in ("fused", "wide", "shade_pipe", "root_cull", "slim_state", "camera_trace", "grid"):
        assert on[2][k] == off[2][k], (k, on[2], off[2])  # the knob moves nothing else
    assert on[2]["fused"] is False and on[3] == off[3] == plain[3]
    oimg, want = oracle(crt, key, desc, depth, spp, world)
    for tag, got in (("camera vertex", on), ("CRT_CAMERA_VERTEX=0", off), ("CRT_CAMERA_TRACE=0", plain)):
        print(tag, dict(zip(COUNTERS, got[1])))
        assert got[1] == want, (tag, dict(zip(COUNTERS, zip(got[1], want))))
        bad = np.argwhere(got[0].view(np.uint32) != oimg.view(np.uint32))
        assert bad.shape[0] == 0, (tag, bad.shape[0], bad[:3])
    on[4].scene.traversal_error()
    return dict(zip(COUNTERS, want)), on


@pytest.mark.parametrize("env,slim,cull", [
    (dict(CRT_WIDE="1"), True, True),                                  # four lanes, root cull, slim survivors
    (dict(CRT_WIDE="1", CRT_LANES="1"), True, True),                   # one lane
    (dict(CRT_WIDE="1", CRT_TAIL_FROM="1"), True, True),               # the survivors go to the k_path tail in the full form
    (dict(CRT_WIDE="1", CRT_NOCLASSIFY_FROM="1"), True, True),         # ... to the plain k_shade in the full form
    (dict(CRT_WIDE="1", CRT_SLIM_STATE="0"), False, True),             # the full four planes between pipelined launches
    (dict(CRT_WIDE="1", CRT_ROOT_CULL="0"), True, False),              # no cull: misses end behind the trace, plane d all the same
    (dict(CRT_WIDE="1", CRT_CAMERA_TRACE="2"), True, True),            # every ray deferred: the append runs onto an empty survivor list
    (dict(CRT_WIDE="1", CRT_CAMERA_TRACE="2", CRT_ROOT_CULL="0"), True, False),
], ids=["default", "one-lane", "tail-from-1", "noclassify-from-1", "full-state", "no-cull", "defer-all", "defer-all-no-cull"])
def test_cornellbox(crt, monkeypatch, env, slim, cull):
    desc = scene_desc(crt, "cornellbox", W, H)
    st, on = three_ways(crt, monkeypatch, "cornellbox32-96", desc, 32, SPP, env)
    assert on[2]["root_cull"] is cull and on[2]["shade_pipe"] is True and on[2]["slim_state"] is slim, on[2]
    assert on[3] == (1 if env.get("CRT_LANES") == "1" else 4)
    assert st["camera_rays"] == W * H * SPP and 0.3 * st["camera_rays"] < st["ended_escaped"] and st["vertices"] > st["camera_rays"] // 2
    assert (W * H * SPP) % 256 == 0 and st["ended_escaped"] % 256 != 0  # full rounds dealt, ragged segments left


def test_depth_1_the_vertex_output_has_no_consumer_but_the_depth_limit(crt, monkeypatch):
    desc = scene_desc(crt, "cornellbox", 64, 36)
    st, on = three_ways(crt, monkeypatch, "depth1", desc, 1, SPP, dict(CRT_WIDE="1"))
    assert st["ended_depth"] > 0 and st["vertices"] + st["ended_escaped"] == st["camera_rays"]  # one vertex per path at most


def test_depth_0_keeps_the_launches_of_before(crt, monkeypatch):
    desc = scene_desc(crt, "cornellbox", 64, 36)
    three_ways(crt, monkeypatch, "depth0", desc, 0, SPP, dict(CRT_WIDE="1"), expect=False, trace_on=False)


def test_a_one_entry_stack_mixes_survivors_and_deferred_rays_in_a_segment(crt, monkeypatch, host):
    """CRT_CAMERA_TRACE=3: rays defer mid-tree, so a segment's round holds hits shaded here, deferred rays and culled rays.
    The eight counters are equal under every form by design, so they cannot tell a deferred ray from a hit; what they give
    is the frame's hits at bounce 0 (depth 1: one vertex per path at most, `vertices`). Which of those defer is taken from
    camera_trace itself, compiled for the host with the same one-entry stack over the image the renderer uploads, on the
    pixel-centre rays of every segment (the dealing: segment b, round r holds samples ((r * grid + b) * 256 ..+256)): at
    least one segment must hold a ray that defers and a ray that hits without deferring."""
    import ora_world
    w, h = 64, 36
    desc = scene_desc(crt, "cornellbox", w, h)
    st, on = three_ways(crt, monkeypatch, "depth1", desc, 1, SPP, dict(CRT_WIDE="1", CRT_CAMERA_TRACE="3"))
    assert 0 < st["vertices"] < st["camera_rays"]
    r = on[4]
    grid, pix = on[2]["grid"], r.pixel_indices()
    o = ora_world.OracleRenderer(desc, crt.usda)
    import ctypes as C
    import ora
    rays = np.zeros((len(pix), 6), np.float32)
    for k, p in enumerate(pix):
        i, j = int(p) % w, int(p) // w
        ray = ora.Ray()
        ora.lib().ora_camera_get_ray(C.byref(o.job.camera), (i + 0.5) / w, (j + 0.5) / h, 0.5, 0.5, 0.0, C.byref(ray))
        rays[k, 0:3] = ray.origin.np()
        rays[k, 3:6] = ray.dir.np()
    status = trace(host, r.scene, rays, mask=1, pstack=1)[0]
    survive = r.scene.root_touched(rays)[0]
    n_act, total = len(pix), len(pix) * SPP
    mixed = 0
    for b in range(grid):  # lanes of one sample each: a lane's batch deals n_act paths
        g = np.arange(b * 256, min((b + 1) * 256, n_act))
        if len(g) == 0:
            break
        s = status[g % n_act][survive[g % n_act]]
        mixed += bool((s == DEFER).any() and (s == HIT).any())
    print("segments (of one lane) whose pixel-centre rays hold both kinds:", mixed, "deferred centre rays:", int((status[survive] == DEFER).sum()))
    assert mixed >= 1 and total == st["camera_rays"]


def _tri_spheres_desc(crt):
    """The tessellated spheres of the traversal benchmarks as an unlit world of three meshes (three materials: the
    pipelined shade kernel's table): a larger tree than the staged window, rays that leave k_camera_vertex's stack."""
    desc = crt.usda.SceneDesc()
    groups = [([], [], 0) for _ in range(3)]
    for k, (v, i) in enumerate(fx.tri_spheres()):
        vs, is_, n = groups[k % 3]
        vs.append(v)
        is_.append(np.asarray(i, np.uint32) + np.uint32(n))
        groups[k % 3] = (vs, is_, n + len(v))
    for k, (vs, is_, _n) in enumerate(groups):
        desc.geoms.append(pc._mesh(np.concatenate(vs), np.concatenate(is_), (0.3 + 0.2 * k, 0.6, 0.8 - 0.2 * k), name="spheres %d" % k))
    desc.camera = dict(lookfrom=np.array([1.0, 2.0, 9.0], np.float32), lookat=np.array([0.0, 0.0, 0.0], np.float32),
                       vup=np.array([0, 1, 0], np.float32), vfov_deg=np.float32(50), aspect=np.float32(64 / 36), aperture=np.float32(0),
                       focus_dist=np.float32(6))
    desc.settings.update(width=64, height=36, max_depth=4, spp=4)
    return desc


@pytest.mark.parametrize("knob", ["1", "3"])
def test_tri_spheres(crt, monkeypatch, knob):
    desc = _tri_spheres_desc(crt)
    st, on = three_ways(crt, monkeypatch, "tri_spheres3", desc, None, SPP, dict(CRT_WIDE="1", CRT_CAMERA_TRACE=knob), world=pc.World(crt.usda))
    assert st["closest_hit"] > st["camera_rays"] and st["ended_escaped"] > 0 and on[2]["shade_pipe"] is True


def test_a_camera_inside_the_bounds(crt, monkeypatch):
    cam = dict(lookfrom=np.array([0.0, 2.0, 1.5], np.float32), lookat=np.array([0.0, 2.0, -1.0], np.float32), vfov_deg=np.float32(60.0))
    desc = scene_desc(crt, "cornellbox", 64, 36, cam)
    st, on = three_ways(crt, monkeypatch, "inside6", desc, 6, SPP, dict(CRT_WIDE="1", CRT_ROOT_CULL="1"))
    assert on[2]["root_cull"] is True and st["vertices"] >= st["camera_rays"]  # every camera ray hits


def test_a_camera_looking_away(crt, monkeypatch):
    """Every camera ray is culled or missed: no survivor, no deferred ray, the first extend and shade see empty segments."""
    desc = scene_desc(crt, "cornellbox", 64, 36, dict(lookat=np.array([0.0, 2.0, 9.0], np.float32)))
    for env in (dict(CRT_WIDE="1"), dict(CRT_WIDE="1", CRT_ROOT_CULL="0")):
        st, on = three_ways(crt, monkeypatch, "away6", desc, 6, SPP, env)
        assert st["closest_hit"] == st["ended_escaped"] == st["camera_rays"] == 64 * 36 * SPP and st["vertices"] == 0


def test_an_emitting_material_takes_its_emission_at_the_first_vertex(crt, monkeypatch):
    """cornellbox with one material that emits and scatters: the table has an emitter, so the survivors carry their
    radiance in the full four planes (no slim state), and a camera path's first vertex adds the emission (emit_here)."""
    desc = scene_desc(crt, "cornellbox", 64, 36)
    dark = scene_desc(crt, "cornellbox", 64, 36)
    k = max(range(len(desc.geoms)), key=lambda g: len(desc.geoms[g].get("idx", ())))  # the mesh with the most triangles
    desc.geoms[k]["material"] = dict(desc.geoms[k]["material"], emission_color=(1.0, 0.75, 0.5), emission_luminance=2.0)
    st, on = three_ways(crt, monkeypatch, "emitter6", desc, 6, SPP, dict(CRT_WIDE="1"))
    assert on[2]["shade_pipe"] is True and on[2]["slim_state"] is False
    ref = render(crt, monkeypatch, dark, 6, SPP, dict(CRT_WIDE="1"))
    assert on[1] == ref[1] and float(on[0].sum()) > float(ref[0].sum())  # the same walk, more light


def test_the_plain_shade_kernel_keeps_k_camera(crt, monkeypatch):
    """CRT_SHADE_PIPE=0: no pipelined first shade, so the form reports off and k_camera runs as before."""
    desc = scene_desc(crt, "cornellbox", 64, 36)
    st, on = three_ways(crt, monkeypatch, "cornellbox6-64", desc, 6, SPP, dict(CRT_WIDE="1", CRT_SHADE_PIPE="0"), expect=False)
    assert on[2]["shade_pipe"] is False and on[2]["camera_trace"] is True
