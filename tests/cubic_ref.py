"""The truth for cubic curve spans (Geometry::CubicCurves), written here because the oracle cannot build curves. It
stands on tests/curve_ref.py, which stays as it is: the leaf test is curve_ref.rounded_cone, the decided / undecided rule,
the 8-ulp window and UNDECIDED_CAP are curve_ref's.

(a) flatness_depth: curve.rs:122-141 in numpy float32 with the exact-exponent rule the host uses in place of f32::log2
    (floor(log2(x) / 2) read from x's binary exponent).
(b) cubic_curve_intersect: curve.rs:166-217 restated literally — a Python recursion over one (ray, span) pair, float32
    scalars, AABB::hit as aabb.rs:24-42 with f32::max / f32::min (np.fmax / np.fmin: a NaN operand is dropped).
(c) cubic_span_pairs: the same walk vectorised over pairs (the recursion's visiting order, one node per pair per step),
    pinned to (b) bit for bit by tests/test_cubic_curves.py. The brute-force scene query runs on it.
(d) CubicRefScene: curve_ref.RefScene plus .cubic(spans, mask) and .sphere(center, radius, mask); one candidate column
    per span in the brute-force query."""
import numpy as np

import curve_ref as cr
from curve_ref import f32, MASK_ALL, INVALID, UNDECIDED_CAP, T_RANGES, MASK_CAMERA, MASK_SHADOW, FLOOR, affine12  # noqa: F401

MAX_DEPTH = 10
SQRT_2 = f32(1.41421356237309504880)
HALF = f32(0.5)


def _a(x):
    return np.asarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------------------------- (a)
def flatness_x(cp, max_width):
    """-> (l0, x) of curve.rs:123-136 in float32; cp (..., 4, 3), max_width (...)."""
    cp, mw = _a(cp), _a(max_width)
    with np.errstate(all="ignore"):
        d0 = (cp[..., 0, :] - cp[..., 1, :] * f32(2.0)) + cp[..., 2, :]
        d1 = (cp[..., 1, :] - cp[..., 2, :] * f32(2.0)) + cp[..., 3, :]
        l0 = np.maximum(np.abs(d0), np.abs(d1)).max(-1)
        eps = mw * f32(0.05)
        x = ((SQRT_2 * f32(6.0)) * l0) / (f32(8.0) * eps)
    return l0, x


def flatness_depth(cp, max_width):
    """curve.rs:122-141 with floor(log2(x) * 0.5) evaluated exactly: floor(floor(log2 x) / 2), floor(log2 x) = x's binary
    exponent. 0 when l0 <= 0, max_width <= 0, x is not finite, or x < 1."""
    l0, x = flatness_x(cp, max_width)
    mw = _a(max_width)
    zero = (l0 <= 0) | (mw <= 0) | ~np.isfinite(x) | ~(x >= 1)
    _m, e = np.frexp(np.where(zero, f32(1.0), x))  # x = m * 2^e, m in [0.5, 1): floor(log2 x) = e - 1
    depth = np.clip((e.astype(np.int64) - 1) // 2, 0, MAX_DEPTH)
    return np.where(zero, 0, depth).astype(np.uint32)


def span_depths(spans):
    s = _a(spans).reshape(-1, 14)
    return flatness_depth(s[:, 0:12].reshape(-1, 4, 3), f32(2.0) * np.maximum(s[:, 12], s[:, 13]))


# ---------------------------------------------------------------------------------------------- (b)
def _vmin(a, b):  # Vec3A::min (minps)
    return np.where(a < b, a, b)


def _vmax(a, b):
    return np.where(a > b, a, b)


def subdivide_bezier(cp):
    """curve.rs:104-112: cp (..., 4, 3) -> (..., 7, 3)."""
    p01 = (cp[..., 0, :] + cp[..., 1, :]) * HALF
    p12 = (cp[..., 1, :] + cp[..., 2, :]) * HALF
    p23 = (cp[..., 2, :] + cp[..., 3, :]) * HALF
    p012 = (p01 + p12) * HALF
    p123 = (p12 + p23) * HALF
    p0123 = (p012 + p123) * HALF
    return np.stack([cp[..., 0, :], p01, p012, p0123, p123, p23, cp[..., 3, :]], -2)


def aabb_hit(mn, mx, o, d, t_min, t_max):
    """aabb.rs:24-42 for one box and one ray (float32 scalars)."""
    with np.errstate(all="ignore"):
        for a in range(3):
            inv_d = f32(1.0) / d[a]
            t0 = (mn[a] - o[a]) * inv_d
            t1 = (mx[a] - o[a]) * inv_d
            if inv_d < 0:
                t0, t1 = t1, t0
            t_min = np.fmax(t_min, t0)
            t_max = np.fmin(t_max, t1)
            if t_max <= t_min:
                return False
    return True


def _subdivide_and_intersect(o, d, cp, u0, u1, r0_full, r1_full, depth, t_min, t_max):
    def radius_at(u):
        return r0_full + (r1_full - r0_full) * u

    if depth == 0:
        hit, t, n = cr.rounded_cone(o, d, cp[0], cp[3], radius_at(u0), radius_at(u1), t_min, t_max)
        return (f32(t), _a(n)) if bool(hit) else None
    split = subdivide_bezier(cp)
    u_mid = (u0 + u1) * HALF
    best = None
    for sub_cp, su0, su1 in ((split[0:4], u0, u_mid), (split[3:7], u_mid, u1)):
        cur_t_max = t_max if best is None else best[0]
        radius = np.fmax(radius_at(su0), radius_at(su1))
        mn = _vmin(_vmin(_vmin(sub_cp[0], sub_cp[1]), sub_cp[2]), sub_cp[3]) - radius
        mx = _vmax(_vmax(_vmax(sub_cp[0], sub_cp[1]), sub_cp[2]), sub_cp[3]) + radius
        if not aabb_hit(mn, mx, o, d, t_min, cur_t_max):
            continue
        hit = _subdivide_and_intersect(o, d, sub_cp, su0, su1, r0_full, r1_full, depth - 1, t_min, cur_t_max)
        if hit is not None:
            best = hit
    return best


def cubic_curve_intersect(o, d, cp, r0, r1, t_min, t_max, depth=None):
    """curve.rs:166-176 for ONE pair: -> None or (t, outward normal). depth: given, it replaces flatness_depth's."""
    o, d, cp = _a(o), _a(d), _a(cp).reshape(4, 3)
    r0, r1, t_min, t_max = f32(r0), f32(r1), f32(t_min), f32(t_max)
    if depth is None:
        depth = int(flatness_depth(cp, f32(2.0) * np.fmax(r0, r1)))
    with np.errstate(all="ignore"):
        return _subdivide_and_intersect(o, d, cp, f32(0.0), f32(1.0), r0, r1, int(depth), t_min, t_max)


# ---------------------------------------------------------------------------------------------- (c)
def cubic_span_pairs(o, d, cp, r0, r1, depth, t_min, t_max):
    """The walk of (b) for N pairs at once: o, d (N, 3); cp (N, 4, 3); r0, r1, depth (N); t_min, t_max scalar or (N).
    -> hit (N) bool, t (N), n (N, 3), zero on a miss. Every pair steps through the recursion's nodes in the recursion's
    order — (level, index) with the control points replayed from the root — so the operations and their order per pair
    are (b)'s."""
    o, d, cp = _a(o).reshape(-1, 3), _a(d).reshape(-1, 3), _a(cp).reshape(-1, 4, 3)
    N = len(o)
    r0, r1 = np.broadcast_to(_a(r0), (N,)), np.broadcast_to(_a(r1), (N,))
    depth = np.broadcast_to(np.asarray(depth, np.int64), (N,))
    t_min, t_max = np.broadcast_to(_a(t_min), (N,)), np.broadcast_to(_a(t_max), (N,))
    found = np.zeros(N, bool)
    t_out = np.zeros(N, np.float32)
    n_out = np.zeros((N, 3), np.float32)
    with np.errstate(all="ignore"):
        z = depth == 0
        if z.any():
            ra, rb = r0[z] + (r1[z] - r0[z]) * f32(0.0), r0[z] + (r1[z] - r0[z]) * f32(1.0)  # radius_at(0), radius_at(1)
            h, t, n = cr.rounded_cone(o[z], d[z], cp[z, 0], cp[z, 3], ra, rb, t_min[z], t_max[z])
            found[z], t_out[z], n_out[z] = h, t, n
        act = np.nonzero(~z)[0]
        level = np.ones(len(act), np.int64)
        idx = np.zeros(len(act), np.int64)
        cur = t_max[act].copy()
        dr = r1 - r0
        while len(act):
            c = cp[act]
            for k in range(int(level.max()) - 1, -1, -1):
                s = subdivide_bezier(c)
                second = ((idx >> k) & 1).astype(bool)
                half = np.where(second[:, None, None], s[:, 3:7], s[:, 0:4])
                c = np.where((level > k)[:, None, None], half, c)
            su0 = np.ldexp(idx.astype(np.float32), -level.astype(np.int32)).astype(np.float32)
            su1 = np.ldexp((idx + 1).astype(np.float32), -level.astype(np.int32)).astype(np.float32)
            ra, rb = r0[act] + dr[act] * su0, r0[act] + dr[act] * su1
            radius = np.fmax(ra, rb)[:, None]
            mn = _vmin(_vmin(_vmin(c[:, 0], c[:, 1]), c[:, 2]), c[:, 3]) - radius
            mx = _vmax(_vmax(_vmax(c[:, 0], c[:, 1]), c[:, 2]), c[:, 3]) + radius
            lo, hi = t_min[act].copy(), cur.copy()
            inside = np.ones(len(act), bool)
            for a in range(3):
                inv_d = f32(1.0) / d[act, a]
                t0, t1 = (mn[:, a] - o[act, a]) * inv_d, (mx[:, a] - o[act, a]) * inv_d
                t0, t1 = np.where(inv_d < 0, t1, t0), np.where(inv_d < 0, t0, t1)
                lo, hi = np.fmax(lo, t0), np.fmin(hi, t1)
                inside &= ~(hi <= lo)
            descend = inside & (level < depth[act])
            leaf = inside & ~descend
            if leaf.any():
                q = act[leaf]
                h, t, n = cr.rounded_cone(o[q], d[q], c[leaf, 0], c[leaf, 3], ra[leaf], rb[leaf], t_min[q], cur[leaf])
                w = q[h]
                found[w], t_out[w], n_out[w] = True, t[h], n[h]
                cur[np.nonzero(leaf)[0][h]] = t[h]
            level = np.where(descend, level + 1, level)
            idx = np.where(descend, idx << 1, idx)
            up = ~descend
            for _ in range(MAX_DEPTH + 1):  # a second half is done: so is its parent
                m = up & ((idx & 1) == 1)
                idx = np.where(m, idx >> 1, idx)
                level = np.where(m, level - 1, level)
            done = up & (level == 0)
            idx = np.where(up & ~done, idx | 1, idx)
            keep = ~done
            act, level, idx, cur = act[keep], level[keep], idx[keep], cur[keep]
    return found, t_out, n_out


def sphere_hit(o, d, center, radius, t_min, t_max):
    """prim.rs:133-161 in float32, vectorised: open range (t_min, t_max). -> hit, t, outward normal."""
    with np.errstate(all="ignore"):
        o, d, c = _a(o), _a(d), _a(center)
        r = f32(radius)
        oc = o - c
        a = cr.dot3(d, d)
        half_b = cr.dot3(oc, d)
        cc = cr.dot3(oc, oc) - r * r
        disc = half_b * half_b - a * cc
        ok = ~(disc < 0)
        sq = np.sqrt(np.where(ok, disc, f32(0)))
        root = (-half_b - sq) / a
        bad = (root <= f32(t_min)) | (root >= f32(t_max))
        root2 = (-half_b + sq) / a
        root = np.where(bad, root2, root)
        ok = ok & ~(bad & ((root2 <= f32(t_min)) | (root2 >= f32(t_max))))
        n = ((o + root[..., None] * d) - c) / r
        return ok, np.where(ok, root, f32(0)), np.where(ok[..., None], n, f32(0))


# ---------------------------------------------------------------------------------------------- (d)
class CubicRefScene(cr.RefScene):
    """curve_ref.RefScene with cubic spans and spheres; build() attaches spans through attach_cubic_curves."""

    def cubic(self, spans, mask=MASK_ALL):
        self.geoms.append(("cubic", np.ascontiguousarray(spans, np.float32).reshape(-1, 14), mask))
        return len(self.geoms) - 1

    def sphere(self, center, radius, mask=MASK_ALL):
        self.geoms.append(("sphere", _a(center), float(radius), mask))
        return len(self.geoms) - 1

    def build(self, api, triangles_only=False):
        b = api.SceneBuilder()
        for g in self.geoms:
            if g[0] == "tris":
                b.attach_triangles(g[1], g[2], None, g[3])
            elif triangles_only:
                b.attach_empty(g[-1])
            elif g[0] == "curves":
                b.attach_round_curves(g[1], g[2])
            elif g[0] == "cubic":
                b.attach_cubic_curves(g[1], g[2])
            elif g[0] == "sphere":
                b.attach_sphere(g[1], g[2], g[3])
            else:
                b.attach_instance(g[1].build(api), g[2], g[3], g[4])
        return b.commit()

    def n_spans(self):
        return sum(len(g[1]) if g[0] == "cubic" else (g[1].n_spans() if g[0] == "inst" and hasattr(g[1], "n_spans") else 0)
                   for g in self.geoms)

    def _candidates(self, o, d, time, mask, t_min, t_max):
        out = super()._candidates(o, d, time, mask, t_min, t_max)  # round segments and instances (which come back here)
        nr = len(o)
        for gid, g in enumerate(self.geoms):
            if g[0] == "cubic":
                sp = g[1]
                ns = len(sp)
                cp = sp[:, 0:12].reshape(ns, 4, 3)
                depth = span_depths(sp)
                rep = lambda x: np.broadcast_to(x[None], (nr,) + x.shape).reshape((nr * ns,) + x.shape[1:])  # noqa: E731
                hit, t, n = cubic_span_pairs(np.repeat(o, ns, 0), np.repeat(d, ns, 0), rep(cp), rep(sp[:, 12]), rep(sp[:, 13]),
                                             rep(depth), f32(t_min), f32(t_max))
                hit = hit.reshape(nr, ns) & ((mask & np.uint32(g[2])) != 0)[:, None]
                out.append((hit, t.reshape(nr, ns), n.reshape(nr, ns, 3), np.full((nr, ns), gid, np.uint32),
                            np.broadcast_to(np.arange(ns, dtype=np.uint32), (nr, ns))))
            elif g[0] == "sphere":
                hit, t, n = sphere_hit(o, d, g[1], g[2], t_min, t_max)
                hit = hit & ((mask & np.uint32(g[3])) != 0)
                out.append((hit[:, None], t[:, None], n[:, None, :], np.full((nr, 1), gid, np.uint32), np.zeros((nr, 1), np.uint32)))
        return out


# ---------------------------------------------------------------------------------------------- inputs
K_CIRCLE = 0.55228475  # curve.rs:337
QUARTER = [(1, 0, 0), (1, K_CIRCLE, 0), (K_CIRCLE, 1, 0), (0, 1, 0)]
STRAIGHT = [(0, 0, 0), (4.0 / 3.0, 0, 0), (8.0 / 3.0, 0, 0), (4, 0, 0)]  # p0.lerp(p3, 1/3), p0.lerp(p3, 2/3): below


def straight_cp():
    """curve.rs:327-329: p0, p0.lerp(p3, 1/3), p0.lerp(p3, 2/3), p3 in float32 (lerp = a + (b - a) * s)."""
    p0, p3 = _a([0, 0, 0]), _a([4, 0, 0])
    return np.stack([p0, p0 + (p3 - p0) * f32(1.0 / 3.0), p0 + (p3 - p0) * f32(2.0 / 3.0), p3])


def deep_span():
    """One span whose flatness depth is exactly 10: a wide zig-zag, hair thin."""
    return np.array([[-4, 1, 0, 4, 3, 0.5, -4, 3, -0.5, 4, 1.5, 0, 1.2e-4, 1.0e-4]], np.float32)


def edge_pairs():
    """The edge list: (labels, rows) with rows of 22 floats o d cp0..cp3 r0 r1 t_min t_max."""
    inf = np.inf
    q = [c for p in QUARTER for c in p]
    # the quarter circle's first half after one split: its hull's faces are where axis-parallel rays start below
    s = subdivide_bezier(_a(QUARTER))
    r = f32(0.05)
    mn = (s[0:4].min(0) - r).astype(np.float32)
    mx = (s[0:4].max(0) + r).astype(np.float32)
    mx2 = (s[3:7].max(0) + r).astype(np.float32)
    on = lambda x: float(np.sqrt(1.0 - float(x) ** 2))  # noqa: E731  (the unit circle's y at x)
    deep = deep_span()[0]
    mid = bezier_points(deep[None], [0.5])[0]
    off = bezier_points(deep[None], [0.3])[0]
    rows = [
        ("arc point, down the z axis (dx = dy = 0: inf * finite, no NaN)", [0.70710678, 0.70710678, 10, 0, 0, -1] + q + [0.05, 0.05, 0.001, inf]),
        ("axis-parallel, origin ON a sub-box face in x (0 * inf = NaN)", [float(mx[0]), 0.3, 10, 0, 0, -1] + q + [0.05, 0.05, 0.001, inf]),
        ("axis-parallel, on the first half's x face, hits in the second half", [float(mn[0]), on(mn[0]), 10, 0, 0, -1] + q + [0.05, 0.05, 0.001, inf]),
        ("axis-parallel, on the second half's x face, hits in the first half", [float(mx2[0]), on(mx2[0]) - 0.02, 10, 0, 0, -1] + q + [0.05, 0.05, 0.001, inf]),
        ("axis-parallel, origin ON a sub-box face in y", [0.9, float(mn[1]), 10, 0, 0, -1] + q + [0.05, 0.05, 0.001, inf]),
        ("axis-parallel along x, origin on the z face", [5, 0.2, float(mx[2]), -1, 0, 0] + q + [0.05, 0.05, 0.001, inf]),
        ("axis-parallel along y through the tube", [1.0, -3, 0.0, 0, 1, 0] + q + [0.05, 0.05, 0.001, inf]),
        ("zero direction", [0.7, 0.7, 10, 0, 0, 0] + q + [0.05, 0.05, 0.001, inf]),
        ("tiny direction", [0.7, 0.7, 10, 0, 0, -1e-21] + q + [0.05, 0.05, 0.001, inf]),
        ("starts inside the tube", [0.70710678, 0.70710678, 0.0, 0.6, 0.8, 0] + q + [0.05, 0.05, 0.001, inf]),
        ("starts inside, along the arc's tangent", [0.70710678, 0.70710678, 0.01, -0.70710678, 0.70710678, 0] + q + [0.05, 0.05, 0.001, inf]),
        ("r0 != r1", [0.70710678, 0.70710678, 10, 0, 0, -1] + q + [0.12, 0.02, 0.001, inf]),
        ("r1 > r0, slanted", [2, 2, 3, -0.4, -0.45, -1] + q + [0.02, 0.15, 0.001, inf]),
        ("chord midpoint misses", [0.5, 0.5, 10, 0, 0, -1] + q + [0.05, 0.05, 0.001, inf]),
        ("t_max before the hit", [0.70710678, 0.70710678, 10, 0, 0, -1] + q + [0.05, 0.05, 0.001, 9.0]),
        ("t_min behind the first hit: the far side", [0.70710678, 0.70710678, 10, 0, 0, -1] + q + [0.05, 0.05, 9.98, inf]),
        ("all points equal", [1, 3, 0, 0, -1, 0] + [1, 0, 0] * 4 + [0.5, 0.5, 0.001, inf]),
        ("all points equal, r differ", [1, 3, 0.1, 0, -1, 0] + [1, 0, 0] * 4 + [0.5, 0.2, 0.001, inf]),
        ("zero radii", [0.70710678, 0.70710678, 10, 0, 0, -1] + q + [0.0, 0.0, 0.001, inf]),
        ("straight span", [2, 3, 0, 0, -1, 0] + list(straight_cp().reshape(-1)) + [0.5, 0.5, 0.001, inf]),
        ("depth 10, aimed at the curve's middle", [mid[0], mid[1], 5, 0, 0, -1] + list(deep[0:12]) + [deep[12], deep[13], 0.001, inf]),
        ("depth 10, aimed at u = 0.3, slanted", [off[0] + 0.6, off[1] - 0.8, off[2] + 2.0, -0.3, 0.4, -1.0] + list(deep[0:12]) + [deep[12], deep[13], 0.001, inf]),
        ("depth 10, grazing along the zig-zag", [-6, 2.2, 0.0, 1, 0.02, 0.001] + list(deep[0:12]) + [deep[12], deep[13], 0.001, inf]),
        ("depth 10, a miss", [0.3, 0.1, 5, 0, 0, -1] + list(deep[0:12]) + [deep[12], deep[13], 0.001, inf]),
    ]
    return [x[0] for x in rows], np.array([x[1] for x in rows], np.float32)


def random_spans(n, rng, bends=(0.0, 0.03, 0.12, 0.5, 1.5), scale=4.0, rmin=0.03, rmax=0.3):
    """n seeded spans: a chord in [-scale, scale]^3, the inner control points on it at 1/3 and 2/3 and pushed off it by
    one of `bends` x the chord's length (depths spread from 0 up); r0 != r1."""
    p0 = rng.uniform(-scale, scale, (n, 3))
    p3 = p0 + rng.normal(0, 1, (n, 3)) * scale * 0.4
    ln = np.linalg.norm(p3 - p0, axis=1, keepdims=True)
    bend = np.asarray(bends)[np.arange(n) % len(bends)][:, None]
    p1 = p0 + (p3 - p0) / 3 + rng.normal(0, 1, (n, 3)) * bend * ln
    p2 = p0 + (p3 - p0) * 2 / 3 + rng.normal(0, 1, (n, 3)) * bend * ln
    r0, r1 = rng.uniform(rmin, rmax, n), rng.uniform(rmin, rmax, n)
    return np.concatenate([p0, p1, p2, p3, r0[:, None], r1[:, None]], 1).astype(np.float32)


def bezier_points(spans, u):
    """Points of the spans at parameters u (float64; for aiming rays only): spans (n, 14), u (n,) -> (n, 3)."""
    cp = np.asarray(spans, np.float64)[:, 0:12].reshape(-1, 4, 3)
    u = np.asarray(u, np.float64)[:, None]
    return (cp[:, 0] * (1 - u) ** 3 + 3 * cp[:, 1] * u * (1 - u) ** 2 + 3 * cp[:, 2] * u * u * (1 - u) + cp[:, 3] * u ** 3)


def random_pairs(n, seed, max_depth=5):
    """Seeded (ray, span) pairs, rows as edge_pairs(): three quarters of the rays aimed at a point of the curve (jittered
    by about a radius), from outside; spans whose depth exceeds max_depth are thickened until it does not."""
    rng = np.random.default_rng(seed)
    sp = random_spans(n, rng)
    for _ in range(8):
        deep = span_depths(sp) > max_depth
        if not deep.any():
            break
        sp[deep, 12:14] *= f32(4.0)
    o = rng.uniform(-5, 5, (n, 3))
    target = bezier_points(sp, rng.uniform(0, 1, n)) + rng.normal(0, 1, (n, 3)) * (np.maximum(sp[:, 12], sp[:, 13])[:, None] * 0.7)
    target = np.where(rng.uniform(0, 1, (n, 1)) < 0.75, target, rng.uniform(-4, 4, (n, 3)))
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([1.0, 1.0, 2.0, 0.37], (n, 1))
    t_max = np.where(rng.uniform(0, 1, n) < 0.8, np.inf, rng.uniform(0.5, 8, n))
    return np.concatenate([o, d, sp, np.full((n, 1), 0.001), t_max[:, None]], 1).astype(np.float32)


def run_pairs(rows, depth=None):
    """cubic_span_pairs on rows of 22 floats; depth defaults to each span's own flatness depth."""
    r = np.asarray(rows, np.float32).reshape(-1, 22)
    if depth is None:
        depth = span_depths(r[:, 6:20])
    return cubic_span_pairs(r[:, 0:3], r[:, 3:6], r[:, 6:18].reshape(-1, 4, 3), r[:, 18], r[:, 19], depth, r[:, 20], r[:, 21])


# ---------------------------------------------------------------------------------------------- scenes
def span_tuft(n, seed, spread=2.0):
    """n seeded single-span curves standing on y = 0 (separate curves: no two share an end sphere): heights 0.4-1.4,
    bends by turns from straight to a hook (depths 0-4), radii 0.02-0.12 with r0 != r1, every fifth with r1 > r0."""
    rng = np.random.default_rng(seed)
    base = np.stack([rng.uniform(-spread, spread, n), rng.uniform(0.0, 0.3, n), rng.uniform(-spread, spread, n)], 1)
    up = rng.normal(0, 1, (n, 3)) * [0.4, 0.0, 0.4] + [0, 1, 0]
    up = up / np.linalg.norm(up, axis=1, keepdims=True)
    h = rng.uniform(0.4, 1.4, (n, 1))
    tip = base + up * h
    bend = np.asarray([0.0, 0.004, 0.03, 0.12, 0.45, 1.1])[np.arange(n) % 6][:, None]
    p1 = base + (tip - base) / 3 + rng.normal(0, 1, (n, 3)) * bend * h
    p2 = base + (tip - base) * 2 / 3 + rng.normal(0, 1, (n, 3)) * bend * h
    r0 = rng.uniform(0.05, 0.12, n)
    r1 = np.maximum(rng.uniform(0.2, 0.9, n) * r0, 0.02)
    swap = np.arange(n) % 5 == 4
    r0, r1 = np.where(swap, r1, r0), np.where(swap, r0, r1)
    return np.concatenate([base, p1, p2, tip, r0[:, None], r1[:, None]], 1).astype(np.float32)


def scene_one():
    """One quarter-circle span (lifted above the floor, r0 != r1; depth 3) over the floor quad."""
    q = _a(QUARTER) + _a([0, 0.4, 0])
    s = CubicRefScene()
    s.triangles(*FLOOR)
    s.cubic(np.concatenate([q.reshape(-1), _a([0.05, 0.03])])[None])
    return s


def scene_tuft(n=64, seed=21):
    """64 spans in three geometries by ray mask over the floor: small enough that direct leaf words occur."""
    sp = span_tuft(n, seed)
    a, b = n // 3, 2 * n // 3
    s = CubicRefScene()
    s.triangles(*FLOOR)
    s.cubic(sp[:a], MASK_CAMERA)
    s.cubic(sp[a:b], MASK_SHADOW)
    s.cubic(sp[b:], MASK_ALL)
    return s


def scene_mixed(seed=31):
    """32 spans + 32 round segments + a sphere + the floor in ONE tree: all three scalar arms meet in a leaf list."""
    s = CubicRefScene()
    s.triangles(*FLOOR)
    s.cubic(span_tuft(32, seed))
    s.curves(cr.tuft(32, seed + 1))
    s.sphere((0.3, 0.9, -0.2), 0.45)
    return s


def scene_instanced(n=64, seed=21):
    """The tuft under two instances over the floor — one moving — and once more a level deeper."""
    proto = CubicRefScene()
    proto.cubic(span_tuft(n, seed))
    mid = CubicRefScene()
    c, sn = np.cos(0.5), np.sin(0.5)
    mid.instance(proto, affine12([[c, 0, sn], [0, 1, 0], [-sn, 0, c]], (0.25, 0, 0)))
    s = CubicRefScene()
    s.triangles(*FLOOR)
    s.instance(proto, affine12(np.diag([0.5, 1.7, 0.8]), (-3, 0, -3)))
    s.instance(proto, affine12(np.eye(3), (3, 0, -3)), affine12(np.eye(3) * 1.1, (3.5, 0.3, -2.5)))
    s.instance(mid, affine12(np.diag([1.2, 0.9, 1.0]), (0, 0, 3)), mask=MASK_ALL)
    return s


def scene_deep():
    s = CubicRefScene()
    s.cubic(deep_span())
    return s


def world_targets(scene, rng, n, time=0.0, along=(0.0, 1.0), xf=None):
    """Per curve geometry below `scene`, points to aim at in world space at a shutter time (float64): on a span at a
    parameter in `along`, on a round segment's axis, each jittered by about the local radius. -> list of (k, 3)."""
    out = []
    for g in scene.geoms:
        pts = None
        if g[0] == "cubic":
            k = rng.integers(0, len(g[1]), n)
            sp = g[1][k].astype(np.float64)
            pts = bezier_points(sp, rng.uniform(along[0], along[1], n)) + rng.normal(0, 1, (n, 3)) * (np.maximum(sp[:, 12], sp[:, 13])[:, None] * 0.6)
        elif g[0] == "curves":
            k = rng.integers(0, len(g[1]), n)
            sg = g[1][k].astype(np.float64)
            u = rng.uniform(along[0], along[1], (n, 1))
            pts = sg[:, 0:3] * (1 - u) + sg[:, 4:7] * u + rng.normal(0, 1, (n, 3)) * (np.maximum(sg[:, 3], sg[:, 7])[:, None] * 0.6)
        elif g[0] == "sphere":
            pts = np.asarray(g[1], np.float64)[None] + rng.normal(0, 1, (n, 3)) * g[2] * 0.6
        elif g[0] == "inst":
            m = g[2].astype(np.float64) if g[3] is None else g[2].astype(np.float64) * (1 - time) + g[3].astype(np.float64) * time
            M, t = m[0:9].reshape(3, 3).T, m[9:12]
            if xf is not None:
                M, t = xf[0] @ M, xf[0] @ t + xf[1]
            out += world_targets(g[1], rng, n, time, along, (M, t))
            continue
        if pts is not None:
            out.append(pts if xf is None else pts @ xf[0].T + xf[1])
    return out


def _has_sphere(scene):
    return any(g[0] == "sphere" or (g[0] == "inst" and _has_sphere(g[1])) for g in scene.geoms)


def scene_rays(scene, n, seed, times=(0.0,), along=(0.0, 1.0), edge=True):
    """n seeded rays, half aimed at the scene's curves (world_targets), half random; masks CAMERA / SHADOW / ALL by turns;
    behind them the edge list's rays (edge_pairs' origins and directions). -> rays8.
    A scene with a sphere gets the edge list without its two rays of no direction: the sphere test (prim.rs:133-161)
    answers those with t = 0 / 0 — a NaN passes both of its range tests, in the reference as on the device — and a NaN
    winner is nothing the brute-force query orders."""
    rng = np.random.default_rng(seed)
    time = np.asarray(times, np.float32)[np.arange(n) % len(times)]
    o = rng.uniform(-6, 6, (n, 3)) * [1, 0.5, 1] + [0, 3.2, 0]
    target = rng.uniform(-5, 5, (n, 3)) * [1, 0.2, 1]
    for tm in np.unique(time):
        sel = np.nonzero((time == tm) & (np.arange(n) % 2 == 0))[0]
        pools = world_targets(scene, rng, len(sel), float(tm), along)
        pick = rng.integers(0, len(pools), len(sel))
        target[sel] = np.stack(pools, 0)[pick, np.arange(len(sel))]
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([1.0, 1.0, 1.0, 2.0, 1e-3], (n, 1))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, time
    masks = np.array([MASK_CAMERA, MASK_SHADOW, MASK_ALL], np.uint32)[(np.arange(n) // 2) % 3]
    rays[:, 7] = masks.view(np.float32)
    if not edge:
        return rays
    labels, e = edge_pairs()
    if _has_sphere(scene):
        e = e[[i for i, l in enumerate(labels) if l not in ("zero direction", "tiny direction")]]
    er = np.zeros((len(e), 8), np.float32)
    er[:, 0:6] = e[:, 0:6]
    er[:, 6] = time[0]
    er[:, 7] = np.array([MASK_ALL], np.uint32).view(np.float32)[0]
    return np.concatenate([rays, er], 0)
