"""A deterministic corpus of scenes and rays at the edges of ray-triangle traversal (no RNG): rays through shared
edges and vertices of integer meshes (exact zeros of the f32 edge functions, the scalar f64 fallback of
triangle.rs:110-172), the same meshes behind exact instance transforms, direction / range / geometry edge cases and
non-finite rays. Every ray carries a label, so a failing comparison names its case.

A scene is a list of geometries (dicts) that `build(api, name)` commits through either builder (the oracle, tests/ora.py,
or the package): {"kind": "mesh", "verts", "idx", "region"}, {"kind": "sphere", "c", "r"}, {"kind": "instance", "scene":
<geometry list>, "l2w", "l2w_end"}. `region` says what the exact reference may demand of a mesh (tests/exact_rt.py):
"flat" a flat connected mesh (watertight away from its outer boundary), "convex" the closed surface of a convex solid,
None nothing beyond its triangles. Instance transforms are exact: integer translations, 90-degree rotations,
uniform power-of-two scales and a mirror, so world-space triangles are exactly the transformed local ones.

Rays: `cases(name)` -> list of Case(label, o, d, time, mask, t_min, t_max). The batched queries take one range per
launch: `groups(cases)` splits a list by range.
"""
from collections import namedtuple

import numpy as np

f32 = np.float32
INF = float("inf")
MASK_ALL = 0xFFFFFFFF
T_MIN = 0.001

Case = namedtuple("Case", "label o d time mask t_min t_max")


# ------------------------------------------------------------------ meshes (integer / dyadic vertices)
def grid_mesh(n, z, lo=0.0, step=1.0):
    """n x n cells in the plane z, two triangles per cell; the diagonal alternates so that shared edges run in all
    three directions. 2 n^2 triangles: the shared edges fall in different Tri4 packets and different leaves."""
    verts = [(lo + i * step, lo + j * step, z) for j in range(n + 1) for i in range(n + 1)]
    idx = []
    for j in range(n):
        for i in range(n):
            a, b = j * (n + 1) + i, j * (n + 1) + i + 1
            c, d = a + n + 1, b + n + 1
            idx += [(a, b, d), (a, d, c)] if (i + j) % 2 == 0 else [(a, b, c), (b, d, c)]
    return np.array(verts, f32), np.array(idx, np.uint32)


def cube_mesh(h, k, c=(0.0, 0.0, 0.0)):
    """The surface of [-h, h]^3 + c, each face a k x k grid, triangles wound outward."""
    verts, idx = [], []
    s = 2.0 * h / k
    for axis in range(3):
        for sign in (-1.0, 1.0):
            u_ax, v_ax = (axis + 1) % 3, (axis + 2) % 3
            if sign < 0:
                u_ax, v_ax = v_ax, u_ax
            base = len(verts)
            for j in range(k + 1):
                for i in range(k + 1):
                    p = [0.0, 0.0, 0.0]
                    p[axis] = sign * h + c[axis]
                    p[u_ax] = -h + i * s + c[u_ax]
                    p[v_ax] = -h + j * s + c[v_ax]
                    verts.append(tuple(p))
            for j in range(k):
                for i in range(k):
                    a, b = base + j * (k + 1) + i, base + j * (k + 1) + i + 1
                    cc, d = a + k + 1, b + k + 1
                    idx += [(a, b, d), (a, d, cc)]
    return np.array(verts, f32), np.array(idx, np.uint32)


def octa_mesh(r, c):
    """The octahedron with vertices c +- r e_i, each face split in four at its edge midpoints, wound outward."""
    verts, idx = [], []
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                p = [(c[0] + sx * r, c[1], c[2]), (c[0], c[1] + sy * r, c[2]), (c[0], c[1], c[2] + sz * r)]
                if sx * sy * sz < 0:
                    p = [p[0], p[2], p[1]]
                m01 = tuple((a + b) / 2 for a, b in zip(p[0], p[1]))
                m12 = tuple((a + b) / 2 for a, b in zip(p[1], p[2]))
                m20 = tuple((a + b) / 2 for a, b in zip(p[2], p[0]))
                base = len(verts)
                verts += [p[0], p[1], p[2], m01, m12, m20]
                idx += [(base, base + 3, base + 5), (base + 3, base + 1, base + 4), (base + 5, base + 4, base + 2),
                        (base + 3, base + 4, base + 5)]
    return np.array(verts, f32), np.array(idx, np.uint32)


def mesh(vi, region=None, mask=MASK_ALL):
    return {"kind": "mesh", "verts": vi[0], "idx": vi[1], "region": region, "mask": mask}


# ------------------------------------------------------------------ exact transforms (glam Affine3A, 12 floats)
def affine(m=None, t=(0.0, 0.0, 0.0)):
    m = np.eye(3) if m is None else np.asarray(m, dtype=np.float64)
    return np.concatenate([m[:, 0], m[:, 1], m[:, 2], np.asarray(t, np.float64)]).astype(f32)


ROT_Z90 = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
ROT_X90 = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
MIRROR_X = [[-1, 0, 0], [0, 1, 0], [0, 0, 1]]


def inst(scene, l2w, l2w_end=None):
    return {"kind": "instance", "scene": scene, "l2w": l2w, "l2w_end": l2w_end, "mask": MASK_ALL}


# ------------------------------------------------------------------ scenes
def _scenes():
    grid = [mesh(grid_mesh(8, 5.0), "flat")]
    closed = [mesh(cube_mesh(2.0, 4), "convex"), mesh(octa_mesh(4.0, (12.0, 0.0, 0.0)), "convex")]
    p_grid = [mesh(grid_mesh(4, 0.0, -2.0), "flat")]  # [-2, 2]^2 at z = 0
    p_cube = [mesh(cube_mesh(1.0, 2), "convex")]
    nested = [inst(p_cube, affine(ROT_X90, (0.0, 0.0, 0.0))), inst(p_grid, affine(None, (0.0, 0.0, 3.0)))]
    instances = [
        inst(p_grid, affine(None, (0.0, 0.0, 5.0))),                                   # translation
        inst(p_grid, affine(ROT_Z90, (20.0, 0.0, 5.0))),                               # 90 degrees about z
        inst(p_cube, affine(np.eye(3) * 2.0, (0.0, 20.0, 0.0))),                       # scale 2
        inst(p_cube, affine(np.eye(3) * 0.5, (20.0, 20.0, 0.0))),                      # scale 1/2
        inst(p_grid, affine(MIRROR_X, (-20.0, 0.0, 5.0))),                             # mirror
        inst(nested, affine(np.eye(3) * 2.0, (0.0, -20.0, 0.0))),                      # two levels
        inst(p_cube, affine(None, (-20.0, 20.0, 0.0)), affine(None, (-20.0, 20.0, 8.0))),  # moving: t=0 / t=1
    ]
    sliver = (np.array([(0, 0, 0), (3, 1, 0), (3 + 2.0 ** -21, 1 + 2.0 ** -23, 0)], f32) + f32(0.0))
    degenerate = [
        # 0: zero-area (a repeated vertex) and collinear triangles, both on the z = 1 plane
        mesh((np.array([(0, 0, 1), (2, 0, 1), (0, 2, 1), (4, 0, 1), (5, 1, 1), (6, 2, 1)], f32),
              np.array([(0, 1, 1), (3, 4, 5), (0, 1, 2)], np.uint32))),
        # 1: a triangle seen edge-on by rays in the plane x = 10 and a face-on one behind it
        mesh((np.array([(10, 0, 0), (10, 2, 0), (10, 0, 2), (9, -1, 3), (11, -1, 3), (9, 3, 3)], f32),
              np.array([(0, 1, 2), (3, 4, 5)], np.uint32))),
        # 2: exactly coincident triangles in one mesh (one packet: the later lane must win, bvh.rs:542)
        mesh((np.array([(20, 0, 1), (22, 0, 1), (20, 2, 1)], f32), np.array([(0, 1, 2), (0, 1, 2)], np.uint32))),
        # 3, 4: the same triangle in two geometries
        mesh((np.array([(20, 4, 1), (22, 4, 1), (20, 6, 1)], f32), np.array([(0, 1, 2)], np.uint32))),
        mesh((np.array([(20, 4, 1), (22, 4, 1), (20, 6, 1)], f32), np.array([(0, 1, 2)], np.uint32))),
        # 5: a sliver whose f32 normal is exactly zero (Tri4::normal_ok = 0, prim.rs:81-83) with a plate behind it;
        #    its f32 edge functions cancel to 0 for rays beside it (the f64 re-evaluation decides, triangle.rs:110-172)
        mesh((np.concatenate([sliver, np.array([(-2, -2, 2), (6, -2, 2), (-2, 6, 2)], f32)]),
              np.array([(0, 1, 2), (3, 4, 5)], np.uint32))),
        {"kind": "sphere", "c": (40.0, 0.0, 0.0), "r": 2.0, "mask": MASK_ALL},
    ]
    return {"grid": grid, "closed": closed, "instances": instances, "degenerate": degenerate}


SCENES = _scenes()
NAMES = list(SCENES)


def build(api, name):
    """Commits scene `name` through `api` (tests/ora.py or the package); instanced scenes are built first and kept."""
    keep = []

    def commit(geoms):
        b = api.SceneBuilder()
        for g in geoms:
            if g["kind"] == "mesh":
                b.attach_triangles(g["verts"], g["idx"], mask=g["mask"])
            elif g["kind"] == "sphere":
                b.attach_sphere(g["c"], g["r"], mask=g["mask"])
            else:
                inner = commit(g["scene"])
                keep.append(inner)
                b.attach_instance(inner, g["l2w"], g["l2w_end"], mask=g["mask"])
        return b.commit()

    return commit(SCENES[name]), keep


# ------------------------------------------------------------------ world-space triangles (exact transforms)
def _apply(m12, p):
    m = np.asarray(m12, np.float64)
    return m[0:3] * p[0] + m[3:6] * p[1] + m[6:9] * p[2] + m[9:12]


def world_triangles(name, time=0.0):
    """[(geom_id, prim_id, region, (v0, v1, v2) as float64 triples, placement)] of the scene at `time` (0 or 1): the
    ids the traversal reports (the top-level geometry, the innermost primitive), the vertices in world space (exact:
    the transforms here only permute, negate, scale by powers of two and translate by integers), and a key naming the
    placed mesh (the path of geometry indices from the top)."""
    out = []

    def walk(geoms, xf, top, path):
        for gi, g in enumerate(geoms):
            gid = gi if top is None else top
            if g["kind"] == "mesh":
                for pi, t in enumerate(g["idx"]):
                    vs = tuple(tuple(float(c) for c in xf(np.asarray(g["verts"][k], np.float64))) for k in t)
                    out.append((gid, pi, g["region"], vs, path + (gi,)))
            elif g["kind"] == "instance":
                m = g["l2w"] if (g["l2w_end"] is None or time <= 0.0) else g["l2w_end"]
                walk(g["scene"], (lambda p, m=m, xf=xf: xf(_apply(m, p))), gid, path + (gi,))
    walk(SCENES[name], lambda p: p, None, ())
    return out


# ------------------------------------------------------------------ rays
AXES = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)]
SLOPES = [(0.25, 0.5, 1.0), (-0.375, 0.125, 1.0), (0.5, -0.5, -1.0), (1.0, 0.25, 0.5), (0.125, -1.0, 0.75)]


def _targets_of(tris, stride=1):
    """Vertices, edge midpoints and centroids-by-quarters (dyadic) of the triangles: the exact points rays aim at."""
    pts = []
    for _g, _p, _r, (a, b, c), _k in tris[::stride]:
        a, b, c = np.array(a), np.array(b), np.array(c)
        pts += [a, (a + b) / 2, (b + c) / 2, (a + b + 2 * c) / 4]
    seen, out = set(), []
    for p in pts:
        key = tuple(p)
        if key not in seen:
            seen.add(key)
            out.append(p)
    return out


def _aim(label, target, d, back, time=0.0, t_min=T_MIN, t_max=INF, scale=1.0):
    d = np.asarray(d, np.float64)
    o = target - back * d
    assert np.array_equal(o.astype(f32).astype(np.float64), o), label  # exact origins: the line passes the target
    return Case(label, o.astype(f32), (d * scale).astype(f32), f32(time), MASK_ALL, t_min, t_max)


def _aimed(prefix, tris, dirs, stride, backs=(6.0,), time=0.0):
    out = []
    for ti, p in enumerate(_targets_of(tris, stride)):
        for di, d in enumerate(dirs):
            for b in backs:
                out.append(_aim("%s/p%d/d%d/b%g" % (prefix, ti, di, b), p, d, b, time))
    return out


def _grid_cases():
    tris = world_triangles("grid")
    out = _aimed("grid/aim", tris, AXES[:2] + SLOPES, 3)
    # every interior vertex and edge midpoint of the grid, straight down and straight up: exact zeros, shared edges
    for j in range(1, 8):
        for i in range(1, 8):
            for dx, dy in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)):
                p = np.array([i + dx, j + dy, 5.0])
                out.append(_aim("grid/down/%g,%g" % (p[0], p[1]), p, (0.0, 0.0, -1.0), 3.0))
                out.append(_aim("grid/up/%g,%g" % (p[0], p[1]), p, (0.0, 0.0, 1.0), 5.0))
    # direction edge cases, aimed at an interior vertex, an edge midpoint and a cell
    tiny = float(np.float32(1e-21)), float(np.float32(3e-21)),
    sub = float(np.float32(1e-45)), float(np.float32(2.0 ** -140))
    for p in (np.array([3.0, 4.0, 5.0]), np.array([3.5, 4.0, 5.0]), np.array([3.25, 4.5, 5.0])):
        tag = "%g,%g" % (p[0], p[1])
        # +-0.0 components, below the 1e-20 safe_inv3 threshold, subnormal (the origin is set 5 below the plane)
        for k, d in enumerate([(0.0, -0.0, 1.0), (-0.0, -0.0, 1.0), (-0.0, 0.0, -1.0), (tiny[0], -tiny[1], 1.0),
                               (-sub[0], sub[1], 1.0), (sub[1], -sub[1], -1.0)]):
            o = p - (5.0 if d[2] > 0 else -5.0) * np.array([0.0, 0.0, 1.0])
            out.append(Case("grid/dir-zero-tiny-sub/%s/%d" % (tag, k), o.astype(f32), np.array(d, f32), f32(0.0),
                            MASK_ALL, T_MIN, INF))
        # exact ties in |d| (the choice of kz, triangle.rs:47-58), a negative dominant axis
        for k, d in enumerate([(1.0, 1.0, 1.0), (-1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (0.5, 0.5, -0.5),
                               (1.0, 1.0, 0.5), (-1.0, 0.0, -1.0), (0.0, 1.0, 1.0)]):
            dd = np.array(d)
            out.append(_aim("grid/dir-tie/%s/%d" % (tag, k), p, dd, 3.0))
        # unnormalised lengths from about 1e-3 to 1e3 (powers of two keep the line through the target; 1e-3 / 1e3
        # themselves do not, the reference allows any length, ray.rs)
        for s in (2.0 ** -10, 1e-3, 2.0 ** 10, 1e3, 1.0 / 3.0):
            out.append(_aim("grid/dir-len/%s/%g" % (tag, s), p, (0.25, -0.5, 1.0), 4.0, scale=s))
    return out


def _range_cases():
    """t_min / t_max exactly at a hit's t (5, exact for these rays) and one ulp either side; t_min == t_max; t_max <
    t_min; t_min = 0 for origins on the plane."""
    five = f32(5.0)
    up, dn = float(np.nextafter(five, f32(INF))), float(np.nextafter(five, f32(0)))
    ranges = [(T_MIN, 5.0), (T_MIN, dn), (T_MIN, up), (5.0, INF), (dn, INF), (up, INF), (5.0, 5.0), (dn, up),
              (6.0, 4.0), (up, dn)]
    out = []
    for p in (np.array([2.0, 3.0, 5.0]), np.array([2.5, 3.0, 5.0]), np.array([2.25, 3.5, 5.0]),
              np.array([4.0, 4.0, 5.0])):
        for k, d in enumerate([(0.0, 0.0, 1.0), (0.25, -0.5, 1.0), (-0.125, 0.375, 1.0)]):
            for lo, hi in ranges:
                c = _aim("range/%g,%g/d%d/[%r,%r]" % (p[0], p[1], k, lo, hi), p, d, 5.0)
                out.append(c._replace(t_min=lo, t_max=hi))
        for k, d in enumerate([(0.0, 0.0, 1.0), (0.5, 0.25, -1.0)]):  # origin ON the plane: t = 0
            out.append(Case("range/on-plane/%g,%g/d%d" % (p[0], p[1], k), p.astype(f32), np.array(d, f32), f32(0.0),
                            MASK_ALL, 0.0, INF))
    return out


def _closed_cases():
    tris = world_triangles("closed")
    out = _aimed("closed/aim", tris, AXES + SLOPES[:3], 5)
    # from inside: the centres and off-centre points, every axis and slope
    for c in (np.array([0.0, 0.0, 0.0]), np.array([0.5, -1.0, 1.5]), np.array([12.0, 0.0, 0.0]),
              np.array([13.0, 1.0, -0.5])):
        for k, d in enumerate(AXES + SLOPES):
            out.append(Case("closed/inside/%g,%g,%g/%d" % (c[0], c[1], c[2], k), c.astype(f32), np.array(d, f32), f32(0.0),
                            MASK_ALL, T_MIN, INF))
    # along cube edges and through cube corners (both faces meet there), from outside
    for p in (np.array([2.0, 2.0, 0.0]), np.array([2.0, 2.0, 2.0]), np.array([-2.0, 1.0, 2.0]), np.array([16.0, 0.0, 0.0]),
              np.array([12.0, 4.0, 0.0]), np.array([14.0, 0.0, 2.0])):
        for k, d in enumerate([(-1.0, -1.0, 0.0), (-1.0, -0.5, -0.25), (-1.0, -1.0, -1.0), (0.5, -1.0, 0.25)]):
            out.append(_aim("closed/edge-vertex/%g,%g,%g/%d" % (p[0], p[1], p[2], k), p, d, 6.0))
    return out


def _instance_cases():
    out = []
    for t in (0.0, 1.0):
        tris = world_triangles("instances", t)
        out += _aimed("inst/t%g" % t, tris, [AXES[0], AXES[1], AXES[2], SLOPES[0], SLOPES[2]], 7, time=t)
    return out


def _degenerate_cases():
    out = []
    for k, p in enumerate([(1.0, 0.0, 1.0), (0.0, 0.0, 1.0), (5.0, 1.0, 1.0), (0.5, 0.5, 1.0), (4.5, 0.5, 1.0)]):
        out.append(_aim("degen/zero-area/%d" % k, np.array(p), (0.0, 0.0, 1.0), 2.0))
    for k, p in enumerate([(10.0, 0.5, 0.5), (10.0, 1.0, 1.0), (10.0, 0.0, 0.0)]):  # in the plane x = 10: edge-on
        for j, d in enumerate([(0.0, 0.0, 1.0), (0.0, 0.5, 1.0), (0.0, 1.0, 0.0)]):
            out.append(_aim("degen/edge-on/%d/%d" % (k, j), np.array(p), d, 2.0))
    for k, p in enumerate([(20.5, 0.5, 1.0), (21.0, 0.0, 1.0), (20.0, 1.0, 1.0), (20.5, 4.5, 1.0), (21.0, 5.0, 1.0)]):
        for j, d in enumerate([(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.25, 0.5, 1.0)]):
            out.append(_aim("degen/coincident/%d/%d" % (k, j), np.array(p), d, 2.0))
    # the sliver: its vertices, points on its long edges, and beside it where f32 cancels an edge function to 0
    y_near = [float(np.nextafter(f32(2.0 / 3.0), f32(k))) for k in (0, 1)] + [float(f32(2.0 / 3.0))]
    for k, p in enumerate([(0.0, 0.0, 0.0), (3.0, 1.0, 0.0), (1.5, 0.5, 0.0), (2.0, y_near[0], 0.0),
                           (2.0, y_near[1], 0.0), (2.0, y_near[2], 0.0), (3.0, 1.0 + 2.0 ** -23, 0.0),
                           (3.0 + 2.0 ** -22, 1.0, 0.0), (1.5 + 2.0 ** -22, 0.5, 0.0),
                           (1.0, float(np.nextafter(f32(1.0 / 3.0), f32(0))), 0.0)]):  # an f32 edge function cancels
        # to 0 where the exact one is < 0: the f64 re-evaluation finds the miss
        for j, d in enumerate([(0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]):
            out.append(Case("degen/sliver/%d/%d" % (k, j), (np.array(p) - 3.0 * np.array(d)).astype(f32),
                            np.array(d, f32), f32(0.0), MASK_ALL, T_MIN, INF))
    # the sphere at (40, 0, 0), r 2: tangent rays (disc == 0), origins inside, through the centre
    for k, (o, d) in enumerate([((38.0, -5.0, 0.0), (0.0, 1.0, 0.0)), ((42.0, 0.0, -5.0), (0.0, 0.0, 1.0)),
                                ((40.0, 2.0, -5.0), (0.0, 0.0, 1.0)), ((40.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
                                ((41.0, 0.5, -0.25), (-0.5, 0.25, 1.0)), ((35.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
                                ((39.0, 0.0, 0.0), (0.0, -1.0, 0.0))]):
        out.append(Case("degen/sphere/%d" % k, np.array(o, f32), np.array(d, f32), f32(0.0), MASK_ALL, T_MIN, INF))
    return out


def _nonfinite_cases(name, p):
    """NaN or +-inf in the origin, the direction or the time. Triangle scenes only: see tests/test_gpu_edge_rays.py."""
    nan, inf = float("nan"), INF
    out = []
    o0, d0 = np.array(p, np.float64) - 4.0 * np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0])
    for k, (o, d, t) in enumerate([
            ((nan, o0[1], o0[2]), d0, 0.0), ((o0[0], nan, o0[2]), d0, 0.0), ((o0[0], o0[1], inf), d0, 0.0),
            ((-inf, o0[1], o0[2]), d0, 0.0), (o0, (nan, 0.0, 1.0), 0.0), (o0, (0.0, 0.0, inf), 0.0),
            (o0, (inf, -inf, 1.0), 0.0), (o0, (0.0, nan, 0.0), 0.0), (o0, (nan, nan, nan), 0.0), (o0, d0, nan),
            (o0, d0, inf), (o0, d0, -inf)]):
        out.append(Case("%s/nonfinite/%d" % (name, k), np.array(o, f32), np.array(d, f32), f32(t), MASK_ALL, T_MIN, INF))
    return out


def cases(name):
    if name == "grid":
        return _grid_cases() + _range_cases() + _nonfinite_cases("grid", (3.5, 4.0, 5.0))
    if name == "closed":
        return _closed_cases() + _nonfinite_cases("closed", (0.5, 0.5, 2.0))
    if name == "instances":
        return _instance_cases() + _nonfinite_cases("instances", (0.5, 0.5, 5.0))
    return _degenerate_cases()


def finite(c):
    return bool(np.isfinite(c.o).all() and np.isfinite(c.d).all() and np.isfinite(c.time))


def rays8(cs):
    """[n, 8] float32: origin, direction, time, mask bits (tests/ora.py, the package's pack_rays)."""
    r = np.zeros((len(cs), 8), f32)
    for i, c in enumerate(cs):
        r[i, 0:3], r[i, 3:6], r[i, 6] = c.o, c.d, c.time
        r[i, 7] = np.array([c.mask], np.uint32).view(f32)[0]
    return r


def groups(cs):
    """{(t_min, t_max): [indices]} in first-seen order: one batched launch per range."""
    out = {}
    for i, c in enumerate(cs):
        out.setdefault((c.t_min, c.t_max), []).append(i)
    return out
