"""The camera rays' one-ray-per-lane traversal (kernels/traverse_camera.hip.h: camera_trace, camera_hit_record — what
k_camera runs) WITHOUT a GPU: the header compiled as host C++ (tests/host_shade/camera_host.cpp) over the image the library
would upload (crt_scene_image.h, crt_scene_image_array), against the oracle's traversal.

The rule: every ray either DEFERS — it is abandoned, and the renderer's first extend traces it with the pool engine — or
returns the oracle's hit bit for bit: t, the ray-facing normal, the geometry word with its front-face bit; a miss is the
oracle's miss. For a ray that does not defer, the oracle's phase trace (ora_set_trace) holds only node and packet steps,
and as many of each as the loop took: the visit order is the reference's, not merely the hit.

So that the test cannot pass by deferring everything: on cornellbox's camera rays the deferred share of the rays that
survive the root cull EQUALS the share of oracle traces that hold a phase other than node / packet (a scalar primitive, an
instance), computed here from the oracle, and that share is below 0.10 (the per-bounce work profile of the scene gives
0.014 descents and 0.01 scalar steps per camera ray, about 0.04 of the survivors). Scenes of triangles alone never defer at
the full stack depth.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fuzz_scenes
import ora
import packet_cases as pc
import scenes
from test_root_cull_host import bounds_of, edge_rays, random_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
T_MIN, INF = 0.001, float("inf")
MISS, HIT, DEFER = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _built():
    ora.build()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("camera_host") / "libcamera_host.so"
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + os.path.join(ROOT, "crust-render_amd", "csrc", "kernels"),
           os.path.join(ROOT, "tests", "host_shade", "camera_host.cpp"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    L = C.CDLL(str(out))
    vp, fp, up = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.camera_host_trace_n.argtypes = [vp] * 7 + [up, fp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_float, C.c_float,
                                                 C.POINTER(C.c_int32), fp, up, up]
    L.camera_host_trace_n.restype = None
    L.camera_host_stack_entries.restype = C.c_int
    return L


def trace(host, p_scene, rays, mask=0xFFFFFFFF, pstack=None):
    """-> status [n], hit record floats [n, 4] (t, ray-facing normal), geometry word [n], (node, packet) steps [n, 2]."""
    arrays, fields = p_scene.image_arrays()
    view = (C.c_uint32 * 8)(*[fields[k] for k in ("root", "has_packets", "n_nodes", "n_packets", "direct_leaves", "pool_stack", "cold")], 0)
    r6 = np.ascontiguousarray(np.asarray(rays, f32)[:, :6])
    n = len(r6)
    status, hit4, gw, steps = np.zeros(n, np.int32), np.zeros((n, 4), f32), np.zeros(n, np.uint32), np.zeros((n, 2), np.uint32)
    ptr = [arrays[k].ctypes.data_as(C.c_void_p) for k in p_scene.IMAGE_ARRAYS]
    host.camera_host_trace_n(*ptr, view, r6.ctypes.data_as(C.POINTER(C.c_float)), n,
                             host.camera_host_stack_entries() if pstack is None else pstack, mask, T_MIN, INF,
                             status.ctypes.data_as(C.POINTER(C.c_int32)), hit4.ctypes.data_as(C.POINTER(C.c_float)),
                             gw.ctypes.data_as(C.POINTER(C.c_uint32)), steps.ctypes.data_as(C.POINTER(C.c_uint32)))
    return status, hit4, gw, steps, fields


def oracle(o_scene, rays, mask=0xFFFFFFFF):
    """Per ray: the oracle's hit (or None) and its phase trace."""
    L = ora.lib()
    L.ora_set_trace.argtypes = [C.c_char_p, C.c_size_t]
    L.ora_trace_len.restype = C.c_size_t
    buf = C.create_string_buffer(1 << 16)
    hits, traces = [], []
    try:
        for r in rays:
            L.ora_set_trace(buf, 1 << 16)
            h = o_scene.intersect(ora.ray(r[0:3], r[3:6], 0.0, mask), T_MIN, INF)
            hits.append(None if h is None else (f32(h.t), h.normal.np().astype(f32), int(h.geom_id), int(h.front_face)))
            traces.append(buf.raw[: L.ora_trace_len()])
    finally:
        L.ora_set_trace(None, 0)
    return hits, traces


def check(host, o_scene, p_scene, rays, label, mask=0xFFFFFFFF, pstack=None, never_defers=False):
    """The rule of the module's docstring on one scene and ray set. -> (deferred [n] bool, traces)"""
    status, hit4, gw, steps, fields = trace(host, p_scene, rays, mask, pstack)
    hits, traces = oracle(o_scene, rays, mask)
    assert len(traces[0]) < (1 << 16) - 1
    for k, (h, tr) in enumerate(zip(hits, traces)):
        what = (label, k, rays[k].tolist(), int(status[k]), tr[:64])
        if status[k] == DEFER:
            continue
        assert set(tr) <= set(b"NP"), what  # only node and packet steps: nothing the loop does not do
        assert (tr.count(b"N"), tr.count(b"P")) == (int(steps[k, 0]), int(steps[k, 1])), what
        if h is None:
            assert status[k] == MISS and gw[k] == 0xFFFFFFFF, what
        else:
            t, nrm, geom, front = h
            assert status[k] == HIT, what
            assert hit4[k, 0].view(np.uint32) == t.view(np.uint32), what
            assert np.array_equal(hit4[k, 1:4].view(np.uint32), nrm.view(np.uint32)), what
            assert int(gw[k]) == (geom | (front << 31)), what
    deferred = status == DEFER
    if never_defers:
        assert not deferred.any(), (label, int(deferred.sum()))
    return deferred, traces


def test_cornellbox_camera_rays(crt, host):
    """Jittered camera rays of cornellbox at 192 x 108: the deferred share of the root cull's survivors is the oracle's
    share of traces with a scalar or instance phase — and small."""
    import ora_world
    w, h = 192, 108
    desc = crt.usda.load(os.path.join(ROOT, "scenes", "cornellbox.usda"), w, h)
    o = ora_world.OracleRenderer(desc, crt.usda)
    p_scene = crt.usda.build_world(desc, crt, crt.default_material)[0]
    pix = crt.shard.shard_pixels(w, h, 0, 1)
    rng = np.random.default_rng(7)
    jit = rng.random((len(pix), 2))
    rays = np.zeros((len(pix), 6), f32)
    for k, p in enumerate(pix):
        i, j = int(p) % w, int(p) // w
        r = ora.Ray()
        ora.lib().ora_camera_get_ray(C.byref(o.job.camera), (i + jit[k, 0]) / w, (j + jit[k, 1]) / h, 0.5, 0.5, 0.0, C.byref(r))
        rays[k, 0:3] = r.origin.np()
        rays[k, 3:6] = r.dir.np()
    assert len(rays) == 20736
    deferred, traces = check(host, o.scene, p_scene, rays, "cornellbox", mask=1)  # CRT_MASK_CAMERA
    survive = p_scene.root_touched(rays)[0]
    other = np.array([not set(t) <= set(b"NP") for t in traces])
    assert not (deferred & ~survive).any() and not (other & ~survive).any()
    share_fn, share_ora = float(deferred[survive].mean()), float(other[survive].mean())
    print("deferred share of %d survivors: function %.4f, oracle %.4f" % (int(survive.sum()), share_fn, share_ora))
    assert np.array_equal(deferred, other)  # ray for ray: the loop defers exactly where the reference leaves node / packet
    assert share_fn == share_ora and 0.0 < share_ora < 0.10, (share_fn, share_ora)


@pytest.mark.parametrize("name", ["masks", "stack"])
def test_packet_cases(crt, host, name):
    """Mixed masks in one packet (per ray mask), 4 / 3 / 2 / 1 hits in one packet, the exact tie, the sliver with a zero
    normal and its f64 fallback lanes: triangles alone, so nothing defers."""
    build = lambda api: pc.World(type("M", (), {"fill_material": staticmethod(lambda m, _d: m)})).build_world(pc.desc(crt.usda, name), api, lambda: None)[0]
    o_scene, p_scene = build(ora), build(crt)
    n = 0
    for mask, rays in pc.rays(name):
        deferred, traces = check(host, o_scene, p_scene, rays, name, mask=mask, never_defers=True)
        n += sum(t.count(b"P") for t in traces)
    assert n > 500  # packets were tested


def test_a_shallow_stack_defers_mid_tree_and_changes_no_answer(crt, host):
    """The stack at one entry: rays defer where a node has more than two children to keep, everything else as before."""
    make = scenes.ALL["shards"][0]
    o_scene, p_scene = make(ora), make(crt)
    lo, hi = bounds_of(p_scene)
    rays = random_rays(np.random.default_rng(3), 3000, lo, hi)
    full, _t = check(host, o_scene, p_scene, rays, "shards", never_defers=False)
    one, _t = check(host, o_scene, p_scene, rays, "shards stack 1", pstack=1)
    assert one.sum() > full.sum() and not one.all()


@pytest.mark.parametrize("name", ["tri_spheres", "mixed"])
def test_recipe_scenes_scalar_primitives_defer(crt, host, name):
    """tri_spheres (tessellated spheres: triangles alone) and mixed (triangles and analytic spheres): every ray that
    reaches a leaf with a scalar entry defers — the rays whose oracle trace holds a scalar step are all among the deferred."""
    make = scenes.ALL[name][0]
    o_scene, p_scene = make(ora), make(crt)
    lo, hi = bounds_of(p_scene)
    rng = np.random.default_rng(5)
    rays = random_rays(rng, 4000, lo, hi)
    deferred, traces = check(host, o_scene, p_scene, rays, name)
    other = np.array([not set(t) <= set(b"NP") for t in traces])
    assert (~other).any() and (~deferred).any()
    if name == "mixed":
        assert other.any()
    assert not (other & ~deferred).any()  # (a deferred ray beyond those: only the stack depth, and that is allowed)
    edge, _odd = edge_rays(rng, p_scene.tree()[0][0], lo, hi)
    check(host, o_scene, p_scene, edge, name + " edge")


@pytest.mark.parametrize("seed", [11, 13])
def test_fuzz_worlds_with_instances(crt, host, seed):
    """A triangle soup, spheres, nested and moving instances under one top-level tree; random rays, and rays with zero
    direction components and origins on the root's box faces."""
    rec = fuzz_scenes.recipe(seed)
    o_scene, _ok = fuzz_scenes.build(ora, rec)
    p_scene, _pk = fuzz_scenes.build(crt, rec)
    lo, hi = bounds_of(p_scene)
    rng = np.random.default_rng(seed)
    deferred, _t = check(host, o_scene, p_scene, random_rays(rng, 4000, lo, hi), "fuzz %d" % seed)
    assert 0 < deferred.sum() < len(deferred)
    edge, _odd = edge_rays(rng, p_scene.tree()[0][0], lo, hi)
    check(host, o_scene, p_scene, edge, "fuzz %d edge" % seed)
