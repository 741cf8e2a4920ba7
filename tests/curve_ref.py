"""The truth for round curve segments (Geometry::RoundCurves), written here because the oracle cannot build curves.

(a) rounded_cone: curve.rs:17-93 restated in numpy float32, vectorised over (ray, segment) pairs. Only elementwise
    float32 + - * / sqrt occur — correctly rounded on the host and on gfx950 (tests/test_gpu_math.py) — in the
    association order of glam's dot ((x*x + y*y) + z*z) and of the reference's expressions. Its bits are the expected bits.
(b) RefScene.query: a brute-force scene query on (a): every segment's own nearest hit in [t_min, t_max], geometry masks
    applied, segments below instances met in local space with the reference's unnormalised direction (prim.rs:345-378) and
    their normals taken back up level by level. Triangles of a RefScene (a floor) are answered by the oracle. A ray is
    DECIDED when its winner has no runner-up within 8 ulp: the visiting order of a BVH then cannot change the answer
    (the shrinking t_max only removes candidates behind the winner). occluded does not depend on order at all.
(c) sd_round_cone: Quilez's signed distance to the solid in float64, to check that (a) describes a rounded cone."""
import numpy as np

f32 = np.float32
MASK_ALL = 0xFFFFFFFF
INVALID = 0xFFFFFFFF
UNDECIDED_ULPS = 8
UNDECIDED_CAP = 0.01  # of a test's rays: a condition on the seeds, not a measurement


def _a(x):
    return np.asarray(x, dtype=np.float32)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ---------------------------------------------------------------------------------------------- (a)
def rounded_cone(o, d, p0, p1, r0, r1, t_min, t_max):
    """o, d, p0, p1: (..., 3); r0, r1, t_min, t_max: (...) — all broadcast together. -> hit (bool), t, n (..., 3)."""
    with np.errstate(all="ignore"):
        o, d, p0, p1 = _a(o), _a(d), _a(p0), _a(p1)
        r0, r1, t_min, t_max = _a(r0), _a(r1), _a(t_min), _a(t_max)
        shape = np.broadcast_shapes(o.shape[:-1], d.shape[:-1], p0.shape[:-1], p1.shape[:-1], r0.shape, r1.shape,
                                    t_min.shape, t_max.shape)
        r0 = np.where(r0 > f32(1e-6), r0, f32(1e-6))
        r1 = np.where(r1 > f32(1e-6), r1, f32(1e-6))
        ln = np.sqrt(dot3(d, d))
        alive = np.broadcast_to(~(ln < f32(1e-20)), shape)
        rd = d / ln[..., None]
        n_min, n_max = t_min * ln, t_max * ln
        ba, oa, ob = p1 - p0, o - p0, o - p1
        rr = r0 - r1
        m0, m1, m2, m3 = dot3(ba, ba), dot3(ba, oa), dot3(ba, rd), dot3(rd, oa)
        m5, m6, m7 = dot3(oa, oa), dot3(ob, rd), dot3(ob, ob)
        found = np.zeros(shape, bool)
        best = np.zeros(shape, np.float32)
        u = np.zeros(shape + (3,), np.float32)
        div = np.ones(shape, np.float32)  # 0 marks a body hit: normalised at the end

        def consider(ok, t, vec, dv):
            nonlocal found, best, u, div
            t = np.broadcast_to(t, shape)
            take = np.broadcast_to(ok, shape) & alive & (t >= n_min) & (t <= n_max) & (~found | (t < best))
            found = found | take
            best = np.where(take, t, best)
            u = np.where(take[..., None], np.broadcast_to(vec, shape + (3,)), u)
            div = np.where(take, np.broadcast_to(dv, shape), div)

        d2 = m0 - rr * rr
        k2 = d2 - m2 * m2
        k1 = (d2 * m3 - m1 * m2) + (m2 * rr) * r0
        k0 = ((d2 * m5 - m1 * m1) + ((m1 * rr) * r0) * f32(2.0)) - (m0 * r0) * r0
        h = k1 * k1 - k0 * k2
        body = (d2 > 0) & (h >= 0) & (np.abs(k2) > f32(1e-12))
        sq = np.sqrt(np.where(h >= 0, h, f32(0)))
        for t in ((-k1 - sq) / k2, (-k1 + sq) / k2):
            y = (m1 - r0 * rr) + t * m2
            consider(body & (y > 0) & (y < d2), t, d2[..., None] * (oa + t[..., None] * rd) - ba * y[..., None], f32(0))
        h0 = (m3 * m3 - m5) + r0 * r0
        sq = np.sqrt(np.where(h0 >= 0, h0, f32(0)))
        for t in (-m3 - sq, -m3 + sq):
            consider(h0 >= 0, t, oa + t[..., None] * rd, r0)
        h1 = (m6 * m6 - m7) + r1 * r1
        sq = np.sqrt(np.where(h1 >= 0, h1, f32(0)))
        for t in (-m6 - sq, -m6 + sq):
            consider(h1 >= 0, t, ob + t[..., None] * rd, r1)
        div = np.where(div == 0, np.sqrt(dot3(u, u)), div)
        t = best / np.broadcast_to(ln, shape)
        n = u / div[..., None]
        return found, np.where(found, t, f32(0)), np.where(found[..., None], n, f32(0))


# ---------------------------------------------------------------------------------------------- (c)
def sd_round_cone(p, a, b, r1, r2):
    """Quilez, sdRoundCone(p, a, b, r1, r2), float64, vectorised."""
    p, a, b = (np.asarray(x, np.float64) for x in (p, a, b))
    r1, r2 = np.asarray(r1, np.float64), np.asarray(r2, np.float64)
    d = lambda x, y: (x * y).sum(-1)  # noqa: E731
    ba = b - a
    l2 = d(ba, ba)
    rr = r1 - r2
    a2 = l2 - rr * rr
    il2 = 1.0 / l2
    pa = p - a
    y = d(pa, ba)
    z = y - l2
    w = pa * l2[..., None] - ba * y[..., None]
    x2 = d(w, w)
    y2, z2 = y * y * l2, z * z * l2
    k = np.sign(rr) * rr * rr * x2
    with np.errstate(invalid="ignore"):
        body = (np.sqrt(x2 * a2 * il2) + y * rr) * il2 - r1
    return np.where(np.sign(z) * a2 * z2 > k, np.sqrt(x2 + z2) * il2 - r2,
                    np.where(np.sign(y) * a2 * y2 < k, np.sqrt(x2 + y2) * il2 - r1, body))


# ---------------------------------------------------------------------------------------------- glam Affine3A, float32
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def affine_inverse(m):
    """m: (..., 12) matrix3 columns x, y, z then translation -> its inverse (Affine3A::inverse, SSE2 path)."""
    m = _a(m)
    x, y, z, t = m[..., 0:3], m[..., 3:6], m[..., 6:9], m[..., 9:12]
    t0, t1, t2 = _cross(y, z), _cross(z, x), _cross(x, y)
    inv = f32(1.0) / dot3(z, t2)
    r0, r1, r2 = t0 * inv[..., None], t1 * inv[..., None], t2 * inv[..., None]  # rows of the inverse
    cx = np.stack([r0[..., 0], r1[..., 0], r2[..., 0]], -1)
    cy = np.stack([r0[..., 1], r1[..., 1], r2[..., 1]], -1)
    cz = np.stack([r0[..., 2], r1[..., 2], r2[..., 2]], -1)
    tr = cx * t[..., 0:1]
    tr = tr + cy * t[..., 1:2]
    tr = tr + cz * t[..., 2:3]
    return np.concatenate([cx, cy, cz, -tr], -1)


def _mat_vec(cols, v):
    r = cols[..., 0:3] * v[..., 0:1]
    r = r + cols[..., 3:6] * v[..., 1:2]
    return r + cols[..., 6:9] * v[..., 2:3]


def _normal_up(w2l, n):
    """prim.rs:327, :360: normalize(w2l.matrix3^T * n)."""
    x, y, z = w2l[..., 0:3], w2l[..., 3:6], w2l[..., 6:9]
    nm = np.concatenate([np.stack([x[..., 0], y[..., 0], z[..., 0]], -1), np.stack([x[..., 1], y[..., 1], z[..., 1]], -1),
                         np.stack([x[..., 2], y[..., 2], z[..., 2]], -1)], -1)
    v = _mat_vec(nm, n)
    with np.errstate(all="ignore"):
        return v / np.sqrt(dot3(v, v))[..., None]


# ---------------------------------------------------------------------------------------------- (b)
class RefScene:
    """A scene description both sides are built from: geometries in attach order (= geometry ids)."""

    def __init__(self):
        self.geoms = []

    def curves(self, segs, mask=MASK_ALL):
        self.geoms.append(("curves", np.ascontiguousarray(segs, np.float32).reshape(-1, 8), mask))
        return len(self.geoms) - 1

    def triangles(self, verts, idx, mask=MASK_ALL):
        self.geoms.append(("tris", _a(verts).reshape(-1, 3), np.asarray(idx, np.uint32).reshape(-1, 3), mask))
        return len(self.geoms) - 1

    def instance(self, scene, l2w, l2w_end=None, mask=MASK_ALL):
        self.geoms.append(("inst", scene, _a(l2w), None if l2w_end is None else _a(l2w_end), mask))
        return len(self.geoms) - 1

    def build(self, api, triangles_only=False):
        """api: the package (curves and all) or, triangles_only, the oracle: curve geometries and instances become empty
        slots, so the geometry ids stay the same."""
        b = api.SceneBuilder()
        for g in self.geoms:
            if g[0] == "tris":
                b.attach_triangles(g[1], g[2], None, g[3])
            elif triangles_only:
                b.attach_empty(g[-1])
            elif g[0] == "curves":
                b.attach_round_curves(g[1], g[2])
            else:
                b.attach_instance(g[1].build(api), g[2], g[3], g[4])
        return b.commit()

    def n_segments(self):
        return sum(len(g[1]) if g[0] == "curves" else (g[1].n_segments() if g[0] == "inst" else 0) for g in self.geoms)

    def _candidates(self, o, d, time, mask, t_min, t_max):
        """Every curve segment's nearest hit for every ray, in this scene's space: lists of columns
        (valid, t, n, geom, prim) with arrays of shape (rays, k)."""
        out = []
        for gid, g in enumerate(self.geoms):
            if g[0] == "curves":
                seg = g[1]
                hit, t, n = rounded_cone(o[:, None, :], d[:, None, :], seg[None, :, 0:3], seg[None, :, 4:7], seg[None, :, 3],
                                         seg[None, :, 7], f32(t_min), f32(t_max))
                hit = hit & ((mask & np.uint32(g[2])) != 0)[:, None]
                out.append((hit, t, n, np.full(hit.shape, gid, np.uint32),
                            np.broadcast_to(np.arange(len(seg), dtype=np.uint32), hit.shape)))
            elif g[0] == "inst":
                inner, l2w, l2w_end, gmask = g[1], g[2], g[3], g[4]
                w2l = np.broadcast_to(affine_inverse(l2w), (len(o), 12))
                if l2w_end is not None:  # prim.rs:285-331: the placements lerped at the ray's time, inverted
                    tm = time[:, None]
                    moved = affine_inverse(l2w[None, :] * (f32(1.0) - tm) + l2w_end[None, :] * tm)
                    w2l = np.where((time > 0)[:, None], moved, w2l)
                lo = _mat_vec(w2l, o) + w2l[:, 9:12]
                ld = _mat_vec(w2l, d)  # unnormalised: local t == world t
                for hit, t, n, _geom, prim in inner._candidates(lo, ld, time, mask, t_min, t_max):
                    hit = hit & ((mask & np.uint32(gmask)) != 0)[:, None]
                    n = _normal_up(w2l[:, None, :], n)
                    out.append((hit, t, np.where(hit[..., None], n, f32(0)), np.full(hit.shape, gid, np.uint32), prim))
        return out

    def query(self, ora, rays8, t_min, t_max):
        """-> dict of per-ray arrays: hit, t, normal (ray-facing), front, u, v, geom, prim, decided, occluded."""
        rays8 = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        o, d, time, mask = rays8[:, 0:3], rays8[:, 3:6], rays8[:, 6], rays8[:, 7].view(np.uint32)
        n = len(rays8)
        cols = self._candidates(o, d, time, mask, t_min, t_max)
        if cols:
            hit, t, nrm, geom, prim = (np.concatenate([c[k] for c in cols], 1) for k in range(5))
        else:
            hit, t, geom, prim = np.zeros((n, 0), bool), np.zeros((n, 0), np.float32), np.zeros((n, 0), np.uint32), np.zeros((n, 0), np.uint32)
            nrm = np.zeros((n, 0, 3), np.float32)
        uv = np.zeros((n, 2), np.float32)
        tri = self.build(ora, triangles_only=True)
        hf, ids, front = tri.intersect_n(rays8, t_min, t_max)
        tocc = tri.occluded_n(rays8, t_min, t_max).astype(bool)
        thit = ids[:, 0] != INVALID
        # the triangles' answer as one more candidate column (already ray-facing: flagged by prim column -1 below)
        hit = np.concatenate([hit, thit[:, None]], 1)
        t = np.concatenate([t, hf[:, 0:1]], 1)
        key = np.where(hit, t, f32(np.inf))
        order = np.argsort(key, axis=1, kind="stable")
        w = order[:, 0]
        rows = np.arange(n)
        any_hit = hit[rows, w]
        is_tri = w == hit.shape[1] - 1
        out_t = np.where(any_hit, key[rows, w], f32(0))
        wc = np.minimum(w, max(hit.shape[1] - 2, 0))
        if nrm.shape[1]:
            cn = nrm[rows, wc]
            cfront = dot3(d, cn) < 0
            cn = np.where(cfront[:, None], cn, -cn)
            cgeom, cprim = geom[rows, wc], prim[rows, wc]
        else:
            cn, cfront = np.zeros((n, 3), np.float32), np.zeros(n, bool)
            cgeom = cprim = np.zeros(n, np.uint32)
        normal = np.where(is_tri[:, None], hf[:, 1:4], cn)
        fr = np.where(is_tri, front.astype(bool), cfront)
        uv = np.where(is_tri[:, None], hf[:, 4:6], uv)
        g = np.where(is_tri, ids[:, 0], cgeom)
        p = np.where(is_tri, ids[:, 1], cprim)
        decided = np.ones(n, bool)
        if hit.shape[1] > 1:
            t1 = key[rows, order[:, 1]]
            gap = _ordered(t1) - _ordered(key[rows, w])
            decided = ~any_hit | ~np.isfinite(t1) | (gap > UNDECIDED_ULPS)
        z = any_hit
        return dict(hit=z, t=out_t, normal=np.where(z[:, None], normal, f32(0)), front=fr & z, u=np.where(z, uv[:, 0], f32(0)),
                    v=np.where(z, uv[:, 1], f32(0)), geom=np.where(z, g, np.uint32(INVALID)), prim=np.where(z, p, np.uint32(INVALID)),
                    decided=decided, occluded=hit[:, :-1].any(1) | tocc)


def _ordered(x):
    """float32 -> int64 whose order is the floats' (differences count ulps)."""
    b = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def compare(ref, hits, occ, what=""):
    """The comparison the issue states: every field of the decided rays with array_equal, occluded for all; at most
    UNDECIDED_CAP of the rays undecided. hits: HIT_DTYPE records; occ: per-ray 0/1."""
    dec = ref["decided"]
    assert (~dec).mean() <= UNDECIDED_CAP, (what, "undecided", int((~dec).sum()), len(dec))
    z = ref["hit"][dec]
    checks = [("geom_id", hits["geom_id"][dec], ref["geom"][dec]), ("prim_id", hits["prim_id"][dec], ref["prim"][dec]),
              ("t", (hits["t"][dec] * z).view(np.uint32), (ref["t"][dec] * z).view(np.uint32)),
              ("normal", (hits["normal"][dec] * z[:, None]).view(np.uint32), (ref["normal"][dec] * z[:, None]).view(np.uint32)),
              ("front_face", hits["front_face"][dec] * z, ref["front"][dec].astype(np.uint32)),
              ("u", (hits["u"][dec] * z).view(np.uint32), (ref["u"][dec] * z).view(np.uint32)),
              ("v", (hits["v"][dec] * z).view(np.uint32), (ref["v"][dec] * z).view(np.uint32))]
    for name, got, want in checks:
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
            raise AssertionError((what, name, len(bad), bad[:5].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist()))
    assert np.array_equal(np.asarray(occ).astype(bool), ref["occluded"]), (what, "occluded",
                                                                          np.nonzero(np.asarray(occ).astype(bool) != ref["occluded"])[0][:8].tolist())


# ---------------------------------------------------------------------------------------------- inputs
def known_answers():
    """curve.rs:227-306, the five rounded_cone tests: (label, o, d, p0, p1, r0, r1, t_min, t_max, expect) with expect =
    None (a miss) or (t, t_tol, normal or None, n_tol)."""
    inf, X, Y, Z = np.inf, (1, 0, 0), (0, 1, 0), (0, 0, 1)
    p0, p1 = (0, 0, 0), (4, 0, 0)
    return [
        ("capsule_axial_hit_at_cap", (-3, 0, 0), X, p0, p1, 0.5, 0.5, 0.001, inf, (2.5, 1e-4, (-1, 0, 0), 1e-4)),
        ("capsule_perpendicular_hit_at_radius", (2, 3, 0), (0, -1, 0), p0, p1, 0.5, 0.5, 0.001, inf, (2.5, 1e-3, Y, 1e-3)),
        ("respects_t_range", (2, 3, 0), (0, -1, 0), p0, p1, 0.5, 0.5, 0.001, 2.0, None),
        ("passes_wide", (2, 3, 2), (0, -1, 0), p0, p1, 0.5, 0.5, 0.001, inf, None),
        ("unnormalized_direction", (2, 3, 0), (0, -2, 0), p0, p1, 0.5, 0.5, 0.001, inf, (1.25, 1e-3, None, 0)),
        ("degenerate_swallowed_sphere", (0, 0, -5), Z, p0, (0.1, 0, 0), 1.0, 0.05, 0.001, inf, (4.0, 1e-3, None, 0)),
    ]


def taper_case():
    """curve.rs:259-277 cone_radius_shrinks_along_axis: the two rays; surf = 3 - t."""
    p0, p1 = (0, 0, 0), (4, 0, 0)
    return [((0.5, 3, 0), (0, -1, 0), p0, p1, 0.5, 0.1), ((3.5, 3, 0), (0, -1, 0), p0, p1, 0.5, 0.1)]


def edge_pairs():
    """The edge list: rows of 16 floats o d p0 r0 p1 r1 t_min t_max, with labels."""
    inf = np.inf
    below = float(np.nextafter(f32(2.5), f32(0)))
    cap = [0, 0, 0, 0.5, 4, 0, 0, 0.5]
    rows = [
        ("swallowed cap (d2 <= 0)", [0, 0, -5, 0, 0, 1, 0, 0, 0, 1.0, 0.1, 0, 0, 0.05, 0.001, inf]),
        ("swallowed cap, equal", [0, 3, 0, 0, -1, 0, 0, 0, 0, 0.5, 0.25, 0, 0, 0.25, 0.001, inf]),
        ("r = 0", [2, 3, 0, 0, -1, 0, 0, 0, 0, 0.0, 4, 0, 0, 0.0, 0.001, inf]),
        ("r0 = 0 only", [1, 3, 0, 0, -1, 0, 0, 0, 0, 0.0, 4, 0, 0, 0.5, 0.001, inf]),
        ("p0 == p1", [1, 3, 0, 0, -1, 0, 1, 0, 0, 0.5, 1, 0, 0, 0.5, 0.001, inf]),
        ("p0 == p1, r differ", [1, 3, 0, 0, -1, 0, 1, 0, 0, 0.5, 1, 0, 0, 0.2, 0.001, inf]),
        ("zero direction", [2, 3, 0, 0, 0, 0] + cap + [0.001, inf]),
        ("tiny direction", [2, 3, 0, 0, -1e-21, 0] + cap + [0.001, inf]),
        ("direction x 2", [2, 3, 0, 0, -2, 0] + cap + [0.001, inf]),
        ("direction x 1e-3", [2, 3, 0, 0, -1e-3, 0] + cap + [0.001, inf]),
        ("along the axis", [-3, 0, 0, 1, 0, 0] + cap + [0.001, inf]),
        ("along the axis, off centre", [-3, 0.25, 0, 1, 0, 0] + cap + [0.001, inf]),
        ("starts inside", [2, 0.1, 0, 0, 1, 0] + cap + [0.001, inf]),
        ("starts inside a cap", [0, 0, 0, -1, 0, 0] + cap + [0.001, inf]),
        ("t_max at the hit", [-3, 0, 0, 1, 0, 0] + cap + [0.001, 2.5]),
        ("t_max one ulp below the hit", [-3, 0, 0, 1, 0, 0] + cap + [0.001, below]),
        ("t_min at the hit", [-3, 0, 0, 1, 0, 0] + cap + [2.5, inf]),
        ("taper, r1 > r0", [3.5, 3, 0, 0, -1, 0, 0, 0, 0, 0.1, 4, 0, 0, 0.5, 0.001, inf]),
        ("behind the origin", [2, 3, 0, 0, 1, 0] + cap + [0.001, inf]),
    ]
    return [r[0] for r in rows], np.array([r[1] for r in rows], np.float32)


def random_pairs(n, seed):
    """Seeded (ray, segment) pairs at the reference's test scale: coordinates in [-4, 4], radii in [0.03, 0.5]; three
    quarters of the rays aimed at a point near the segment, from outside it. Rows as edge_pairs()."""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(-4, 4, (n, 3))
    p1 = rng.uniform(-4, 4, (n, 3))
    r0, r1 = rng.uniform(0.03, 0.5, n), rng.uniform(0.03, 0.5, n)
    o = rng.uniform(-4, 4, (n, 3))
    s = rng.uniform(0, 1, (n, 1))
    target = p0 + (p1 - p0) * s + rng.normal(0, 1, (n, 3)) * (np.maximum(r0, r1)[:, None] * 0.7)
    target = np.where(rng.uniform(0, 1, (n, 1)) < 0.75, target, rng.uniform(-4, 4, (n, 3)))
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([1.0, 1.0, 2.0, 0.37], (n, 1))
    t_max = np.where(rng.uniform(0, 1, n) < 0.8, np.inf, rng.uniform(0.5, 8, n))
    return np.concatenate([o, d, p0, r0[:, None], p1, r1[:, None], np.full((n, 1), 0.001), t_max[:, None]], 1).astype(np.float32)


def run_pairs(rows):
    r = np.asarray(rows, np.float32)
    return rounded_cone(r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 10:13], r[:, 9], r[:, 13], r[:, 14], r[:, 15])


FLOOR = (np.array([[-6, 0, -6], [6, 0, -6], [6, 0, 6], [-6, 0, 6]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
MASK_CAMERA, MASK_SHADOW = 1, 2


def tuft(n, seed, spread=2.0):
    """n seeded segments standing on y = 0: lengths 0.2-1, radii 0.03-0.3 tapering, every fifth with r1 > r0."""
    rng = np.random.default_rng(seed)
    base = np.stack([rng.uniform(-spread, spread, n), rng.uniform(0.0, 0.5, n), rng.uniform(-spread, spread, n)], 1)
    dirn = rng.normal(0, 1, (n, 3)) * [0.6, 0.0, 0.6] + [0, 1, 0]
    dirn = dirn / np.linalg.norm(dirn, axis=1, keepdims=True)
    tip = base + dirn * rng.uniform(0.2, 1.0, (n, 1))
    r0 = rng.uniform(0.05, 0.3, n)
    r1 = rng.uniform(0.03, 1.0, n) * r0
    r1 = np.maximum(r1, 0.03)
    swap = np.arange(n) % 5 == 4
    r0, r1 = np.where(swap, r1, r0), np.where(swap, r0, r1)
    return np.concatenate([base, r0[:, None], tip, r1[:, None]], 1).astype(np.float32)


def affine12(m3, t):
    m = np.asarray(m3, np.float32)
    return np.concatenate([m[:, 0], m[:, 1], m[:, 2], np.asarray(t, np.float32)]).astype(np.float32)


def scene_one():
    s = RefScene()
    s.curves(np.array([[0, 0, 0, 0.3, 1, 0.5, 0, 0.1]], np.float32))
    return s


def scene_tuft(n=257, seed=11):
    """Three tufts by ray mask over a two-triangle floor: packets and scalar lists in one tree, more than 255 segments."""
    seg = tuft(n, seed)
    a, b = n // 3, 2 * n // 3
    s = RefScene()
    s.triangles(*FLOOR)
    s.curves(seg[:a], MASK_CAMERA)
    s.curves(seg[a:b], MASK_SHADOW)
    s.curves(seg[b:], MASK_ALL)
    return s


def scene_instanced(n=257, seed=11):
    """The tuft placed three times over the floor: under a non-uniform scale, as a moving instance, two levels deep."""
    proto = RefScene()
    proto.curves(tuft(n, seed))
    mid = RefScene()
    c, sn = np.cos(0.5), np.sin(0.5)
    mid.instance(proto, affine12([[c, 0, sn], [0, 1, 0], [-sn, 0, c]], (0.25, 0, 0)))
    s = RefScene()
    s.triangles(*FLOOR)
    s.instance(proto, affine12(np.diag([0.5, 1.7, 0.8]), (-3, 0, -3)))
    s.instance(proto, affine12(np.eye(3), (3, 0, -3)), affine12(np.eye(3) * 1.1, (3.5, 0.3, -2.5)))
    s.instance(mid, affine12(np.diag([1.2, 0.9, 1.0]), (0, 0, 3)), mask=MASK_ALL)
    return s


def world_segments(scene, time=0.0, xf=None):
    """Segment end points in world space at a shutter time (float64; for aiming rays only)."""
    out = []
    for g in scene.geoms:
        if g[0] == "curves":
            p = g[1].astype(np.float64)
            pts = np.concatenate([p[:, 0:3], p[:, 4:7]], 0)
            if xf is not None:
                pts = pts @ xf[0].T + xf[1]
            out.append(pts)
        elif g[0] == "inst":
            m = g[2].astype(np.float64) if g[3] is None else g[2].astype(np.float64) * (1 - time) + g[3].astype(np.float64) * time
            M, t = m[0:9].reshape(3, 3).T, m[9:12]
            if xf is not None:
                M, t = xf[0] @ M, xf[0] @ t + xf[1]
            out += world_segments(g[1], time, (M, t))
    return out


def scene_rays(scene, n, seed, times=(0.0,), along=None):
    """n seeded rays, half aimed at segment end points (jittered), half random; masks CAMERA / SHADOW / ALL by turns; the
    edge list's rays behind them. -> rays8. along = (lo, hi) aims at points that far along each segment's axis instead:
    for polylines, whose consecutive segments share their end sphere — a hit there is a tie of two segments by
    construction, and so undecided."""
    rng = np.random.default_rng(seed)
    time = np.asarray(times, np.float32)[np.arange(n) % len(times)]
    o = rng.uniform(-6, 6, (n, 3)) * [1, 0.5, 1] + [0, 3.2, 0]
    target = rng.uniform(-5, 5, (n, 3)) * [1, 0.2, 1]
    for tm in np.unique(time):
        ends = world_segments(scene, float(tm))
        pts = np.concatenate(ends, 0)
        if along is not None:
            a = np.concatenate([e[:len(e) // 2] for e in ends], 0)
            b = np.concatenate([e[len(e) // 2:] for e in ends], 0)
        sel = np.nonzero((time == tm) & (np.arange(n) % 2 == 0))[0]
        if along is not None:
            k = rng.integers(0, len(a), len(sel))
            pts = a[k] + (b[k] - a[k]) * rng.uniform(along[0], along[1], (len(sel), 1))
        else:
            pts = pts[rng.integers(0, len(pts), len(sel))]
        target[sel] = pts + rng.normal(0, 0.05, (len(sel), 3))
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([1.0, 1.0, 1.0, 2.0, 1e-3], (n, 1))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, time
    masks = np.array([MASK_CAMERA, MASK_SHADOW, MASK_ALL], np.uint32)[(np.arange(n) // 2) % 3]
    rays[:, 7] = masks.view(np.float32)
    _labels, e = edge_pairs()
    er = np.zeros((len(e), 8), np.float32)
    er[:, 0:6] = e[:, 0:6]
    er[:, 6] = time[0]
    er[:, 7] = np.array([MASK_ALL], np.uint32).view(np.float32)[0]
    return np.concatenate([rays, er], 0)


T_RANGES = ((0.001, float("inf")), (0.5, 6.0), (0.0, 3.0))
