"""Exact ray-triangle reference in rational arithmetic (fractions.Fraction): test infrastructure only.

For a finite ray o + t d and a triangle (v0, v1, v2), all given as f32 values (exact rationals), `evaluate` solves
o + t d = (1 - u - v) v0 + u v1 + v v2 exactly and returns t, the barycentrics and the bounds below. Spheres are not
covered (the corpus's sphere cases are compared with the oracle only).

Error bounds of the f32 watertight test (triangle.rs:41-80 shear, :110-172 edge functions; the oracle's
tri_intersect_sheared and tri4_intersect, the kernels' tri_scalar and packet loop, all with -ffp-contract=off). Let
u = 2^-24 (unit roundoff), R = max_i |v_i - o|_inf, kz the dominant axis of d (|d_kx|, |d_ky| <= |d_kz|, so |s_x|,
|s_y| <= 1), Z = R / |d_kz|, and DET = E0 + E1 + E2 the exact sheared determinant (twice the area of the triangle
projected along d onto the kx-ky plane, DET = n.d / d_kz for n = (v1 - v0) x (v2 - v0)).
 * Sheared coordinates a_x = (v_kx - o_kx) - s_x (v_kz - o_kz): one rounding in each difference, in s_x, in the
   product and in the outer difference, so |da_x| <= (2|a_kx| + 3|s_x a_kz| + 2 R) u <= 7 u R, and |a_x| <= 2 R.
   We take delta = 8 u R (the second-order terms are below u R).
 * Edge function e = b_x c_y - b_y c_x, |b|, |c| <= 2 R: inputs 4 (2R)(delta) = 64 u R^2, the two products
   2 u (2R)^2 = 8 u R^2, the difference u 2 (2R)^2 = 8 u R^2: |de| <= 80 u R^2 = B_e. The f64 re-evaluation of an
   exactly-zero edge function has a smaller error than the f32 one (exact products, one rounding), so B_e bounds it too.
 * Barycentrics. The test accepts only edge functions of one sign, so the exact E_i is >= -B_e on the accepted side,
   and |det - DET| <= 3 B_e + 2 u |DET|: lambda_i >= -TOL_B with TOL_B = B_e / (|DET| - 3 B_e - 2 u |DET|) (infinite when
   the denominator is not positive: the test may then accept anything near the triangle's plane).
 * t = t_s / det, t_s = sum e_i (s_z a_kz,i) with |s_z a_kz,i| <= Z and a relative error of 3 u in s_z a_kz,i:
   |dt_s| <= 3 B_e Z + 3 u Z S + 3 u Z S' where S = sum |E_i| <= |DET| + 6 B_e (one sign up to B_e) and S' <= S + 3 B_e
   the computed one, then the quotient: |dt| <= (|dt_s| + |t| |d det|) / (|DET| - |d det|) + u |t| = TOL_T.
 * The range test compares t_s against t_min |det| and t_max |det| (one rounding each): a hit is certainly inside
   [t_min, t_max] when t is inside by TOL_T + 2 u max(|t_min|, |t_max|, |t|) (infinite bounds: no margin).

When the ray's sheared coordinates come out of f32 exactly (axis or dyadic directions, integer or dyadic vertices and
origins) only the products and differences of the edge functions round, and rounding is monotonic: a computed f32
edge function has the exact sign or is 0, and a 0 is re-evaluated in f64 with exact products. The hit / miss decision is
then EXACT (`decided`): hit iff every lambda_i >= 0 (edges included) and DET != 0. When moreover t_s, det and
t_min |det|, t_max |det| are exact in f32 (`range_decided`), the range test is exact and inclusive (triangle.rs:160-166).
"""
from fractions import Fraction as F

import numpy as np

f32 = np.float32
U = F(1, 2 ** 24)
INF = float("inf")


def fr(x):
    return F(float(x))


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def shear_axes(d):
    """kx, ky, kz as triangle.rs:47-58 chooses them (ties: the later axis; a negative d_kz swaps kx and ky)."""
    ax, ay, az = abs(d[0]), abs(d[1]), abs(d[2])
    kz = (0 if ax > az else 2) if ax > ay else (1 if ay > az else 2)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    if d[kz] < 0:
        kx, ky = ky, kx
    return kx, ky, kz


class Eval:
    __slots__ = ("t", "u", "v", "det", "tol_b", "tol_t", "decided", "range_decided", "parallel")

    def lam(self):
        return (1 - self.u - self.v, self.u, self.v)

    def inside(self, tol=0):
        return not self.parallel and min(self.lam()) >= -tol

    def in_range(self, t_min, t_max, margin):
        lo = self.t >= fr(t_min) + margin if np.isfinite(t_min) else True
        hi = self.t <= fr(t_max) - margin if np.isfinite(t_max) else True
        return lo and hi

    def margin(self, t_min, t_max):
        m = max([abs(x) for x in (t_min, t_max) if np.isfinite(x)] + [abs(float(self.t))])
        return self.tol_t + 2 * U * fr(m)

    def certain(self, t_min, t_max):
        """The f32 test must accept this triangle (before the traversal's closest-hit bound), and the traversal must
        reach it: the point is strictly inside (a point on the outer edge of a mesh can lie on a node box's face, and a
        ray in that face with a zero direction component misses the box, bvh.rs:662-668 with :790-808)."""
        if self.parallel:
            return False
        if not min(self.lam()) > (0 if self.decided else self.tol_b):
            return False  # strictly inside only: on an edge the traversal may reach it through a neighbour, or not at all
        if self.range_decided:
            return self.in_range(t_min, t_max, 0)
        return self.in_range(t_min, t_max, self.margin(t_min, t_max))

    def possible(self, t_min, t_max):
        """The f32 test may accept this triangle."""
        if self.parallel:
            return self.tol_b == INF  # an exactly edge-on triangle: det == 0 unless the computation is unbounded
        if not self.inside(0 if self.decided else self.tol_b):
            return False
        if self.range_decided:
            return self.in_range(t_min, t_max, 0)
        return self.in_range(t_min, t_max, -self.margin(t_min, t_max))


def _f32_sheared(o, d, vs):
    """The sheared coordinates, edge functions, det and t_s as the oracle computes them (float32, its operation order),
    for the exactness flags only."""
    with np.errstate(all="ignore"):
        o32, d32 = np.asarray(o, f32), np.asarray(d, f32)
        kx, ky, kz = shear_axes([float(x) for x in d32])
        sx, sy, sz = d32[kx] / d32[kz], d32[ky] / d32[kz], f32(1.0) / d32[kz]
        co = []
        for v in vs:
            a = np.asarray(v, f32) - o32
            co.append((a[kx] - sx * a[kz], a[ky] - sy * a[kz], sz * a[kz]))
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = co
        e = [bx * cy - by * cx, cx * ay - cy * ax, ax * by - ay * bx]
        if e[0] == 0 or e[1] == 0 or e[2] == 0:
            e = [f32(float(bx) * float(cy) - float(by) * float(cx)), f32(float(cx) * float(ay) - float(cy) * float(ax)),
                 f32(float(ax) * float(by) - float(ay) * float(bx))]
        det = e[0] + e[1] + e[2]
        ts = e[0] * az + e[1] * bz + e[2] * cz
    return (kx, ky, kz), (sx, sy, sz), co, e, det, ts


def evaluate(o, d, vs, t_min=0.0, t_max=INF):
    """Exact intersection of the ray's line with the triangle and the f32 test's bounds (module docstring)."""
    O = tuple(fr(x) for x in o)
    D = tuple(fr(x) for x in d)
    V = [tuple(fr(x) for x in v) for v in vs]
    e1, e2 = _sub(V[1], V[0]), _sub(V[2], V[0])
    n = _cross(e1, e2)
    den = _dot(D, n)
    r = Eval()
    (kx, ky, kz), (sx, sy, sz), co, e, det32, ts32 = _f32_sheared(o, d, vs)
    R = max(abs(c) for v in V for c in _sub(v, O))
    Be = 80 * U * R * R
    r.parallel = den == 0
    if r.parallel:
        r.t = r.u = r.v = r.det = F(0)
        r.tol_b = INF if Be > 0 else 0
        r.tol_t = INF
        r.decided = r.range_decided = False
        return r
    t = _dot(_sub(V[0], O), n) / den
    p = _sub(tuple(O[i] + t * D[i] for i in range(3)), V[0])
    nn = _dot(n, n)
    r.t, r.u, r.v = t, _dot(_cross(p, e2), n) / nn, _dot(_cross(e1, p), n) / nn
    DET = den / D[kz]
    r.det = DET
    dd = 3 * Be + 2 * U * abs(DET)
    Z = R / abs(D[kz])
    S = abs(DET) + 6 * Be
    if abs(DET) - dd > 0:
        r.tol_b = Be / (abs(DET) - dd)
        dts = 3 * Be * Z + 3 * U * Z * S + 3 * U * Z * (S + 3 * Be)
        r.tol_t = (dts + abs(t) * dd) / (abs(DET) - dd) + U * abs(t)
    else:
        r.tol_b = r.tol_t = INF
    # exactness: the f32 sheared coordinates (and then t_s, det and the range products) equal the exact values
    finite = all(np.isfinite(np.float64(x)) for c in co for x in c) and np.isfinite(np.float64(sz))
    exact_co = []
    for v in V:
        a = _sub(v, O)
        exact_co.append((a[kx] - fr(sx) * a[kz], a[ky] - fr(sy) * a[kz], fr(sz) * a[kz]))
    r.decided = bool(finite and fr(sx) == D[kx] / D[kz] and fr(sy) == D[ky] / D[kz]
                     and all(fr(c[i]) == x[i] for c, x in zip(co, exact_co) for i in range(2)))
    r.range_decided = False
    if r.decided:
        E = [exact_co[1][0] * exact_co[2][1] - exact_co[1][1] * exact_co[2][0],
             exact_co[2][0] * exact_co[0][1] - exact_co[2][1] * exact_co[0][0],
             exact_co[0][0] * exact_co[1][1] - exact_co[0][1] * exact_co[1][0]]
        TS = sum(E[i] * exact_co[i][2] for i in range(3))
        bounds = [x for x in (t_min, t_max) if np.isfinite(x)]
        with np.errstate(all="ignore"):
            prods = [f32(x) * abs(det32) for x in bounds]
        r.range_decided = bool(
            all(fr(e[i]) == E[i] for i in range(3)) and fr(det32) == sum(E) and fr(ts32) == TS
            and all(exact_co[i][2] == fr(co[i][2]) for i in range(3))
            and all(fr(p_) == fr(x) * abs(sum(E)) for p_, x in zip(prods, bounds)))
    return r


def candidates(o, d, tris, slack=1e-3):
    """Indices of the triangles whose bounding box the ray's line meets (float64, padded by `slack` of the box's size)
    in the triangle's plane, or which lie nearly parallel to the ray: the only ones worth the exact evaluation."""
    V = np.array(tris, np.float64)  # [n, 3, 3]
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    den = n @ d
    lo, hi = V.min(axis=1), V.max(axis=1)
    pad = slack * (1.0 + np.abs(hi - lo).max(axis=1, keepdims=True) + np.abs(lo).max(axis=1, keepdims=True))
    with np.errstate(all="ignore"):
        t = ((V[:, 0] - o) * n).sum(1) / den
        p = o + t[:, None] * d
        near = ((p >= lo - pad) & (p <= hi + pad)).all(axis=1)
        near_par = np.abs(den) <= 1e-9 * np.linalg.norm(n, axis=1) * np.linalg.norm(d)
    return np.nonzero(near | near_par | ~np.isfinite(t))[0]


def expectations(c, tris):
    """For one finite corpus ray over the scene's world triangles (edge_rays.world_triangles): the exact evaluations
    of the candidate triangles {index: Eval}, and the points where a hit is REQUIRED, [(t, tolerance)]: a triangle the
    f32 test must accept, or a point of a watertight region's surface inside the range by the margin (a flat mesh
    away from its outer edges; a convex closed mesh the line passes through, not one it only touches)."""
    idx = candidates(c.o, c.d, [t[3] for t in tris])
    evs = {int(i): evaluate(c.o, c.d, tris[i][3], c.t_min, c.t_max) for i in idx}
    required = [(ev.t, ev.tol_t) for ev in evs.values() if ev.certain(c.t_min, c.t_max)]
    by_mesh = {}
    for i, ev in evs.items():
        if tris[i][2] is not None and ev.inside(0):
            by_mesh.setdefault(tris[i][4], []).append(i)
    for key, ids in by_mesh.items():
        region = tris[ids[0]][2]
        ts = sorted(set(evs[i].t for i in ids))
        if region == "convex" and not (len(ts) >= 2 and _strictly_inside(tris, key, c, (ts[0] + ts[-1]) / 2)):
            continue  # the line only touches the surface, or runs in it
        bnd = _boundary_edges(tris, key) if region == "flat" else set()
        for tv in ts:
            at = [i for i in ids if evs[i].t == tv]
            if region == "flat" and _on_boundary(evs, tris, at, bnd):
                continue
            tol = max(evs[i].tol_t for i in at)
            if tol == INF:
                continue
            margin = tol + 2 * U * fr(max([abs(x) for x in (c.t_min, c.t_max) if np.isfinite(x)] + [abs(float(tv))]))
            lo_ok = tv >= fr(c.t_min) + margin if np.isfinite(c.t_min) else True
            hi_ok = tv <= fr(c.t_max) - margin if np.isfinite(c.t_max) else True
            if lo_ok and hi_ok:
                required.append((tv, tol))
    return evs, required


_BND = {}


def _strictly_inside(tris, key, c, t):
    """o + t d lies strictly inside the convex closed mesh `key` (strictly on one side of every face's plane)."""
    O, D = [fr(x) for x in c.o], [fr(x) for x in c.d]
    p = tuple(O[i] + t * D[i] for i in range(3))
    signs = set()
    for tr in tris:
        if tr[4] != key:
            continue
        V = [tuple(fr(x) for x in v) for v in tr[3]]
        s = _dot(_cross(_sub(V[1], V[0]), _sub(V[2], V[0])), _sub(p, V[0]))
        signs.add((s > 0) - (s < 0))
    return len(signs) == 1 and 0 not in signs


def _boundary_edges(tris, key):
    k = (id(tris), key)
    if k not in _BND:
        count = {}
        for t in tris:
            if t[4] != key:
                continue
            vs = t[3]
            for a, b in ((vs[0], vs[1]), (vs[1], vs[2]), (vs[2], vs[0])):
                e = (min(a, b), max(a, b))
                count[e] = count.get(e, 0) + 1
        _BND[k] = {e for e, n in count.items() if n == 1}
    return _BND[k]


def _on_boundary(evs, tris, at, bnd):
    """The exact point lies on an outer edge (or an outer vertex) of its flat mesh."""
    for i in at:
        vs = tris[i][3]
        lam = evs[i].lam()
        for j, (a, b) in enumerate(((vs[1], vs[2]), (vs[2], vs[0]), (vs[0], vs[1]))):  # the edge opposite vertex j
            if lam[j] == 0 and (min(a, b), max(a, b)) in bnd:
                return True
    return False


def check(c, tris, hit, t_rep, key_rep, occluded):
    """Problems (strings) with one ray's answers against the exact reference: hit (bool), t_rep (float), key_rep
    ((geom_id, prim_id)), occluded (bool). Empty when the answers are admissible."""
    evs, required = expectations(c, tris)
    bad = []
    if required:
        t_req, tol = min(required, key=lambda x: x[0] + x[1])
        if not hit:
            bad.append("watertight: no hit, exact hit required at t=%g" % float(t_req))
        elif fr(t_rep) > t_req + tol:
            bad.append("closest: t=%r, exact hit at t=%g (tolerance %.3g)" % (t_rep, float(t_req), float(tol)))
        if not occluded:
            bad.append("watertight: not occluded, exact hit required at t=%g" % float(t_req))
    if hit:
        cand = [i for i, t in enumerate(tris) if (t[0], t[1]) == tuple(key_rep)]
        ok = False
        for i in cand:
            ev = evs[i] if i in evs else evaluate(c.o, c.d, tris[i][3], c.t_min, c.t_max)
            if ev.possible(c.t_min, c.t_max) and (ev.tol_t == INF or abs(fr(t_rep) - ev.t) <= ev.tol_t):
                ok = True
        if not ok:
            bad.append("false hit: %s at t=%r is not hit within the bounds" % (tuple(key_rep), t_rep))
    if occluded and not any(ev.possible(c.t_min, c.t_max) for ev in evs.values()):
        if not any(evaluate(c.o, c.d, t[3], c.t_min, c.t_max).possible(c.t_min, c.t_max) for t in tris):
            bad.append("false occlusion")
    return bad
