"""The renderer's root cull as a host function (crt.h, crt_scene_root_touched_n; dev_image.h, node_touched) against
the oracle's traversal. No GPU: the function the generate kernel runs is compiled for the CPU from the same source.

The rule: a camera ray is finished in generate iff it touches no child box of the image's root node. The oracle says the
same thing its own way: the ray's phase trace (ora_set_trace) is exactly one node step, "N", and the query reports no hit.
The two must agree ray for ray — a ray the function calls a miss that the traversal would have carried on with is a wrong
pixel; a ray it keeps although the traversal ends at the root is only a lost saving, but the expressions are the same, so
the test asks for equality.

Rays carry the mask ALL: the oracle writes a trace character for a scalar primitive only after its mask test, so a ray of
a narrower mask that reaches a leaf of masked-out spheres also traces "N"; the root step itself never looks at a mask.

NaN directions are checked apart. A NaN in a slab is dropped by the device's v_max_f32 / v_min_f32 (and by fminf / fmaxf
on the host) but kept by the reference's SSE max when it is the second operand (tests/test_gpu_edge_rays.py), so on such
a ray the oracle steps differently from the engine — and in a scene with spheres it can even report a hit the engine never
looks for, which is why the edge corpus keeps non-finite rays to triangle scenes. There the function is held against a
float32 evaluation with the engine's semantics written here (numpy fmin / fmax, every scene), and, in the scenes made of
triangles only, against the one-sided property that matters: what the function culls, the oracle misses.
"""
import ctypes as C
import os

import numpy as np
import pytest

import fuzz_scenes
import ora
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
T_MIN, INF = 0.001, float("inf")


@pytest.fixture(scope="module", autouse=True)
def _built():
    ora.build()


def oracle_root_miss(o_scene, rays):
    """bool [n]: the oracle's trace of the ray is exactly one node step and the query reports no hit."""
    L = ora.lib()
    L.ora_set_trace.argtypes = [C.c_char_p, C.c_size_t]
    L.ora_trace_len.restype = C.c_size_t
    buf = C.create_string_buffer(4096)
    out = np.zeros(len(rays), bool)
    try:
        for k, r in enumerate(rays):
            L.ora_set_trace(buf, 4096)
            hit = o_scene.intersect(ora.ray(r[0:3], r[3:6]), T_MIN, INF)
            out[k] = hit is None and buf.raw[: L.ora_trace_len()] == b"N"
    finally:
        L.ora_set_trace(None, 0)
    return out


def numpy_root_touched(node_words, rays):
    """node_touched in float32 numpy, sharing no code with the library: safe_inv3 (bvh.rs:662-668), slab4 (bvh.rs:790-808)
    with the NaN-dropping min / max of the device, lane on iff tn <= tf and the lane is valid (WideNode::flags)."""
    bmin = node_words[0:12].view(f32).reshape(3, 4)
    bmax = node_words[12:24].view(f32).reshape(3, 4)
    valid = [(int(node_words[28]) >> l) & 1 for l in range(4)]
    o, d = rays[:, 0:3].astype(f32), rays[:, 3:6].astype(f32)
    with np.errstate(all="ignore"):
        inv = np.where(np.abs(d) < f32(1e-20), np.copysign(f32(1e20), d), f32(1.0) / d).astype(f32)
        any_on = np.zeros(len(rays), bool)
        for l in range(4):
            t0 = ((bmin[:, l][None, :] - o) * inv).astype(f32)
            t1 = ((bmax[:, l][None, :] - o) * inv).astype(f32)
            lo, hi = np.fmin(t0, t1), np.fmax(t0, t1)
            tn = np.fmax(np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2]), f32(T_MIN))
            tf = np.fmin(np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2]), f32(INF))
            if valid[l]:
                any_on |= tn <= tf
    return any_on


def random_rays(rng, n, lo, hi):
    """Origins in a shell of one to four scene sizes around the scene, aimed into a region twice its size: hits, near
    misses and plain misses of the root's boxes all occur."""
    c, e = (lo + hi) / 2, max(float(np.max(hi - lo)), 1e-3)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = c + u * rng.uniform(0.3, 4.0, (n, 1)) * e   # some origins inside the bounds
    t = c + rng.uniform(-1.0, 1.0, (n, 3)) * e
    d = t - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(f32)


def edge_rays(rng, node_words, lo, hi):
    """Rays built from the root node's own numbers: zero direction components, origins exactly on a child box's face, a
    direction parallel to a face at the face's coordinate, infinite directions. -> finite-slab rays, NaN-direction rays."""
    bmin = node_words[0:12].view(f32).reshape(3, 4)
    bmax = node_words[12:24].view(f32).reshape(3, 4)
    lanes = [l for l in range(4) if (int(node_words[28]) >> l) & 1]
    e = max(float(np.max(hi - lo)), 1e-3)
    out = []
    base = random_rays(rng, 64, lo, hi)
    for r in base:  # one and two zero components, both signs of zero
        for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2)):
            for z in (0.0, -0.0):
                q = r.copy()
                q[3 + np.array(axes)] = z
                if np.any(q[3:6] != 0):
                    out.append(q)
    for l in lanes:
        cmin, cmax = bmin[:, l], bmax[:, l]
        mid = ((cmin + cmax) / 2).astype(f32)
        for a in range(3):
            for face in (cmin[a], cmax[a]):
                on = mid.copy()
                on[a] = face  # exactly on the face
                for d in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 1], [-1, -1, -1], [1, -1, 0.5]):
                    out.append(np.concatenate([on, np.array(d, f32)]))
                # parallel to the face at the face's coordinate, from outside the box along another axis, both ways
                b = (a + 1) % 3
                off = on.copy()
                off[b] = cmin[b] - f32(0.75) * f32(e)
                for s in (1.0, -1.0):
                    d = np.zeros(3, f32)
                    d[b] = s
                    out.append(np.concatenate([off, d]))
                # ... and on an edge of the box: two coordinates on faces
                edge = on.copy()
                edge[b] = cmax[b]
                for d in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, -1, -1]):
                    out.append(np.concatenate([edge, np.array(d, f32)]))
    for r in base[:16]:  # infinite components: 1 / inf = 0, no NaN in a slab of finite boxes
        for d in ([INF, 0, 0], [0, -INF, 0], [INF, -INF, 1], [1, 1, INF], [INF, INF, INF]):
            out.append(np.concatenate([r[0:3], np.array(d, f32)]))
    nan = float("nan")
    odd = []
    for r in base[:32]:
        for d in ([nan, r[4], r[5]], [r[3], nan, r[5]], [r[3], r[4], nan], [nan, nan, r[5]], [nan, nan, nan], [nan, 0.0, 1.0], [INF, nan, 0.0]):
            odd.append(np.concatenate([r[0:3], np.array(d, f32)]))
    return np.array(out, f32), np.array(odd, f32)


def check_scene(crt, o_scene, p_scene, rays, label):
    """-> culled share. Finite-slab rays: the function against the oracle's trace, ray for ray."""
    touched, root = p_scene.root_touched(rays)
    assert root is not None, label
    want = oracle_root_miss(o_scene, rays)
    bad = np.nonzero(touched == want)[0]  # culled = not touched
    assert bad.size == 0, (label, bad.size, rays[bad[:3]])
    # and the independent float32 evaluation (the host tree's root is node 0, bvh.rs:442-447)
    nodes = p_scene.tree()[0]
    assert np.array_equal(touched, numpy_root_touched(nodes[0], rays)), label
    return float(np.mean(~touched))


def check_nan_rays(o_scene, p_scene, odd, label, triangles_only=False):
    touched, _root = p_scene.root_touched(odd)
    nodes = p_scene.tree()[0]
    assert np.array_equal(touched, numpy_root_touched(nodes[0], odd)), label
    for r in odd[~touched] if triangles_only else []:  # one direction only: what the function culls, the oracle misses
        assert o_scene.intersect(ora.ray(r[0:3], r[3:6]), T_MIN, INF) is None, (label, r)


def bounds_of(p_scene):
    b = np.asarray(p_scene.bounds(), dtype=np.float64).reshape(2, 3)
    return b[0], b[1]


def test_cornellbox_camera_rays(crt):
    """Jittered camera rays of cornellbox at 192 x 108 in tile order: the oracle alone gives a culled share of 0.444 at
    this shape (the bench's 531 -> 295 M paths after bounce 0), and the function's share is the oracle's, ray for ray."""
    import ora_world
    w, h = 192, 108
    desc = crt.usda.load(os.path.join(ROOT, "scenes", "cornellbox.usda"), w, h)
    o = ora_world.OracleRenderer(desc, crt.usda)
    p_scene = crt.usda.build_world(desc, crt, crt.default_material)[0]
    pix = crt.shard.shard_pixels(w, h, 0, 1)
    rng = np.random.default_rng(7)
    jit = rng.random((len(pix), 2))
    rays = np.zeros((len(pix), 6), f32)
    L = ora.lib()
    for k, p in enumerate(pix):
        i, j = int(p) % w, int(p) // w
        r = ora.Ray()
        L.ora_camera_get_ray(C.byref(o.job.camera), (i + jit[k, 0]) / w, (j + jit[k, 1]) / h, 0.5, 0.5, 0.0, C.byref(r))
        rays[k, 0:3] = r.origin.np()
        rays[k, 3:6] = r.dir.np()
    assert len(rays) == 20736
    touched, root = p_scene.root_touched(rays)
    want = oracle_root_miss(o.scene, rays)
    oracle_share = float(np.mean(want))
    print("culled share: oracle %.4f, function %.4f" % (oracle_share, float(np.mean(~touched))))
    assert root is not None
    assert 0.43 < oracle_share < 0.46, oracle_share  # the scene's own figure: the test cannot pass by culling nothing
    assert np.array_equal(~touched, want)
    assert float(np.mean(~touched)) == oracle_share
    # of all the oracle's misses, only a handful get past the root
    hits = np.array([o.scene.intersect(ora.ray(r[0:3], r[3:6])) is not None for r in rays[::8]])
    assert np.mean(~hits) - np.mean(want[::8]) < 0.01


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_fuzz_recipes_instanced_roots(crt, seed):
    """The fuzz recipes' worlds: a triangle soup, spheres, nested and moving instances under one top-level tree, so the
    root's children are inner nodes and leaves of instances. 10 000 random rays and the edge rays of the root's boxes."""
    rec = fuzz_scenes.recipe(seed)
    o_scene, _ok = fuzz_scenes.build(ora, rec)
    p_scene, _pk = fuzz_scenes.build(crt, rec)
    lo, hi = bounds_of(p_scene)
    rng = np.random.default_rng(seed)
    share = check_scene(crt, o_scene, p_scene, random_rays(rng, 10000, lo, hi), "fuzz %d random" % seed)
    assert 0.02 < share < 0.98, share  # both answers occur
    edge, odd = edge_rays(rng, p_scene.tree()[0][0], lo, hi)
    check_scene(crt, o_scene, p_scene, edge, "fuzz %d edge" % seed)
    check_nan_rays(o_scene, p_scene, odd, "fuzz %d nan" % seed)


def _few_spheres(api):
    b = api.SceneBuilder()
    b.attach_sphere((-3.0, 0.0, 0.0), 0.5)
    b.attach_sphere((3.0, 1.0, 0.5), 0.75)
    inner = api.SceneBuilder()
    inner.attach_sphere((0.0, 0.0, 0.0), 1.0)
    b.attach_instance(inner.commit(), api.affine(t=(0.0, 4.0, -2.0)))
    return b.commit()


@pytest.mark.parametrize("name", ["few_spheres", "mixed", "tri_spheres", "shards", "instances"])
def test_recipe_scenes_and_a_root_with_empty_lanes(crt, name):
    make = _few_spheres if name == "few_spheres" else scenes.ALL[name][0]
    o_scene, p_scene = make(ora), make(crt)
    root_words = p_scene.tree()[0][0]
    if name == "few_spheres":
        assert (int(root_words[28]) & 0xF) != 0xF, "this scene is here for a root with empty lanes"
    lo, hi = bounds_of(p_scene)
    rng = np.random.default_rng(5)
    share = check_scene(crt, o_scene, p_scene, random_rays(rng, 10000, lo, hi), name + " random")
    assert 0.02 < share < 0.98, share
    edge, odd = edge_rays(rng, root_words, lo, hi)
    check_scene(crt, o_scene, p_scene, edge, name + " edge")
    check_nan_rays(o_scene, p_scene, odd, name + " nan", triangles_only=name in ("tri_spheres", "shards"))


def test_an_empty_scene_has_no_root(crt):
    b = crt.SceneBuilder()
    b.attach_empty()
    s = b.commit()
    touched, root = s.root_touched(np.array([[0, 0, 5, 0, 0, -1]], f32))
    assert root is None and not touched.any()
