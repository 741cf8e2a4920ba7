"""Closed forms of image formation: which pixel gets what. float64, numpy and scipy only; nothing here imports the
package's kernels or the oracle. tests/image_cases.py builds the scenes these speak about, tests/test_image_formation.py
holds the CPU oracle to them and tests/test_gpu_image_formation.py the device.

Everything is stated in CAMERA-PLANE PIXEL COORDINATES (x, y): the focus plane of Camera::new (camera.rs:27-60), scaled
so that the frame is [0, width] x [0, height]. x = s * width runs along `horizontal` (+u), y = t * height along
`vertical` (+v); frame position (s, t) = (0, 0) is `lower_left_corner`. Buffer pixel (i, j), stored at j * width + i,
samples x = i + fx, y = j + fy (tracer.rs:574-575), fx and fy being the filter's offsets (filter.rs:193-205; 0.5 is the
pixel centre): row j = 0 looks along lower_left. The conventions this pins: vfov is the VERTICAL angle, aspect is
width / height of the viewport, `aperture` is the lens DIAMETER (camera.rs:49), the filter's sample weight is 1 (so a
pixel's expectation is the integral of the scene under the offsets' density, whatever the radius).

A half-plane is (nx, ny, c) with nx^2 + ny^2 = 1: the lit side is nx * x + ny * y >= c.

`python tests/image_ref.py` runs the module's own checks (self_test)."""
import math

import numpy as np
from scipy import integrate


# ---------------------------------------------------------------- the camera, camera.rs:27-84 in float64 ----------------------------------------------------------------
def camera_frame(cam):
    """Camera::new in float64 -> dict(origin, u, v, w, horizontal, vertical, lower_left, lens_radius, focus)."""
    o, at, up = (np.asarray(cam[k], np.float64) for k in ("lookfrom", "lookat", "vup"))
    w = (o - at) / np.linalg.norm(o - at)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    focus = float(cam["focus_dist"])
    viewport_height = 2.0 * math.tan(math.radians(float(cam["vfov_deg"])) / 2.0)  # vfov: the vertical angle
    viewport_width = float(cam["aspect"]) * viewport_height
    horizontal, vertical = focus * viewport_width * u, focus * viewport_height * v
    return dict(origin=o, u=u, v=v, w=w, horizontal=horizontal, vertical=vertical, focus=focus,
                lower_left=o - horizontal / 2 - vertical / 2 - focus * w, lens_radius=float(cam["aperture"]) / 2.0)


def focus_point(cam, s, t):
    """The point of the focus plane at frame position (s, t)."""
    f = camera_frame(cam)
    return f["lower_left"] + s * f["horizontal"] + t * f["vertical"]


def camera_ray(cam, s, t, lens=(0.0, 0.0)):
    """get_ray (camera.rs:71-84) with the lens point explicit: `lens` is the point of the unit disc, scaled here by the
    lens radius along (u, v). -> (origin, direction, not normalised)."""
    f = camera_frame(cam)
    offset = f["lens_radius"] * (lens[0] * f["u"] + lens[1] * f["v"])
    return f["origin"] + offset, focus_point(cam, s, t) - f["origin"] - offset


def plane_point(cam, x, y, width, height, d):
    """Where the PINHOLE ray through pixel coordinates (x, y) crosses the plane at distance d along the view axis."""
    f = camera_frame(cam)
    return f["origin"] + (d / f["focus"]) * (focus_point(cam, x / width, y / height) - f["origin"])


def pixel_size(cam, width, height):
    """Side of a pixel on the focus plane; the pixels must be square (aspect = width / height)."""
    f = camera_frame(cam)
    px, py = np.linalg.norm(f["horizontal"]) / width, np.linalg.norm(f["vertical"]) / height
    assert abs(px / py - 1.0) < 1e-6, (px, py)
    return float(py)


def lens_blur(cam, width, height, d):
    """A ray from lens point x_l through focus-plane point x_f crosses the plane at distance d at lateral position
    x_l (1 - d/f) + x_f d/f (similar triangles, exact for planes perpendicular to the axis). Divided by the pinhole
    scale d/f and the pixel size: x_f + b * (x_l / R) in pixels, b = R (1 - d/f) f / (d p): the SIGNED blur radius in
    focus-plane pixels (negative behind the focus plane: the blur disc is mirrored)."""
    f = camera_frame(cam)
    return f["lens_radius"] * (1.0 - d / f["focus"]) * f["focus"] / (d * pixel_size(cam, width, height))


# ---------------------------------------------------------------- the filters, filter.rs:193-205 ----------------------------------------------------------------
def filter_support(kind, r):
    return 0.5 - r, 0.5 + r


def filter_cdf(kind, r, x):
    """CDF at x of the sampled offset: uniform on [0.5 - r, 0.5 + r] (box), the tent of half-width r about 0.5 (triangle)."""
    z = (float(x) - 0.5) / r
    if z <= -1.0:
        return 0.0
    if z >= 1.0:
        return 1.0
    if kind == "box":
        return (z + 1.0) / 2.0
    if kind == "triangle":
        return (1.0 + z) ** 2 / 2.0 if z < 0.0 else 1.0 - (1.0 - z) ** 2 / 2.0
    raise ValueError(kind)


def filter_pdf(kind, r, x):
    z = (float(x) - 0.5) / r
    if abs(z) >= 1.0:
        return 0.0
    if kind == "box":
        return 0.5 / r
    if kind == "triangle":
        return (1.0 - abs(z)) / r
    raise ValueError(kind)


def _box_cdf_integral(r, z):
    """Integral of the box CDF from -infinity to z."""
    lo, hi = filter_support("box", r)
    return 0.0 if z <= lo else ((z - lo) ** 2 / (4.0 * r) if z <= hi else z - 0.5)


# ---------------------------------------------------------------- coverage ----------------------------------------------------------------
def clip_area(poly, half_plane):
    """Area of the part of a convex polygon [(x, y), ...] on the lit side of the half-plane (Sutherland-Hodgman, shoelace)."""
    nx, ny, c = half_plane
    out = []
    for k in range(len(poly)):
        a, b = poly[k], poly[(k + 1) % len(poly)]
        da, db = nx * a[0] + ny * a[1] - c, nx * b[0] + ny * b[1] - c
        if da >= 0.0:
            out.append(a)
        if (da > 0.0 > db) or (da < 0.0 < db):
            t = da / (da - db)
            out.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
    area = 0.0
    for k in range(len(out)):
        a, b = out[k], out[(k + 1) % len(out)]
        area += a[0] * b[1] - b[0] * a[1]
    return abs(area) / 2.0


def coverage_polygon(pixel, half_plane):
    """Exact area fraction of the box-0.5 footprint [i, i+1] x [j, j+1] of buffer pixel (i, j) on the lit side."""
    i, j = pixel
    return clip_area([(i, j), (i + 1.0, j), (i + 1.0, j + 1.0), (i, j + 1.0)], half_plane)


def _side(pixel, half_plane, kind, r):
    """+1 / -1 where the whole footprint of the pixel's offsets lies on the lit / dark side, 0 where the edge crosses it."""
    i, j = pixel
    nx, ny, c = half_plane
    lo, hi = filter_support(kind, r)
    d = [nx * (i + a) + ny * (j + b) - c for a in (lo, hi) for b in (lo, hi)]
    return 1 if min(d) >= 0.0 else (-1 if max(d) <= 0.0 else 0)


def edge_coverage(pixel, half_plane, kind="box", r=0.5):
    """P(nx (i + fx) + ny (j + fy) >= c), fx and fy independent with the filter's density: the pixel's expected share of
    the lit side. Exactly 0.0 or 1.0 where the footprint lies on one side. Axis-aligned edges: a closed form of the CDF.
    Any other edge: the product-density integral, the inner one by the CDF, the outer one by scipy's adaptive rule with
    the density's and the inner CDF's breakpoints named."""
    side = _side(pixel, half_plane, kind, r)
    if side:
        return 1.0 if side > 0 else 0.0
    i, j = pixel
    nx, ny, c = half_plane
    beyond = lambda n, z: 1.0 - filter_cdf(kind, r, z) if n > 0.0 else filter_cdf(kind, r, z)  # P(n * offset >= n * z)
    if ny == 0.0:
        return beyond(nx, c / nx - i)
    if nx == 0.0:
        return beyond(ny, c / ny - j)
    lo, hi = filter_support(kind, r)
    xs = lambda y: (c - ny * (j + y)) / nx - i  # the edge's x offset in the row at offset y
    f = lambda y: filter_pdf(kind, r, y) * beyond(nx, xs(y))
    breaks = [0.5] + [(c - nx * (i + x)) / ny - j for x in (lo, 0.5, hi)]
    breaks = sorted(b for b in breaks if lo < b < hi)
    val, _err = integrate.quad(f, lo, hi, points=breaks or None, epsabs=1e-12, epsrel=1e-12, limit=200)
    return min(max(val, 0.0), 1.0)


def lens_edge_coverage(pixel, half_plane, kind, r, blur):
    """The edge on a plane at distance d seen through a thin lens: `blur` = lens_blur(...). With a = n . x_l / R the
    lens point's coordinate across the edge, the ray through focus-plane point x lands on the lit side where
    n . x >= c - blur * a. The lens point is uniform on a disc, which is isotropic: a has the chord density
    (2 / pi) sqrt(1 - a^2) on [-1, 1] whatever the edge's orientation, so the coverage is ONE quadrature of the pinhole
    coverage over a (a = sin(theta), weight (2 / pi) cos^2(theta): no endpoint singularity). blur = 0 (d = f) is the
    pinhole coverage itself."""
    nx, ny, c = half_plane
    pinhole = coverage_polygon if (kind, r) == ("box", 0.5) else (lambda p, h: edge_coverage(p, h, kind, r))
    if blur == 0.0:
        return pinhole(pixel, half_plane)
    b = abs(blur)  # the chord density is even
    sides = [_side(pixel, (nx, ny, c + s * b), kind, r) for s in (-1.0, 1.0)]
    if sides[0] == sides[1] != 0:
        return 1.0 if sides[0] > 0 else 0.0
    f = lambda th: (2.0 / math.pi) * math.cos(th) ** 2 * pinhole(pixel, (nx, ny, c - b * math.sin(th)))
    lo, hi = filter_support(kind, r)  # where the shifted edge enters and leaves the footprint: the integrand's kinks
    reach = [nx * (pixel[0] + x) + ny * (pixel[1] + y) for x in (lo, hi) for y in (lo, hi)]
    kinks = sorted(math.asin(a) for a in ((c - min(reach)) / b, (c - max(reach)) / b) if -1.0 < a < 1.0)
    val, _err = integrate.quad(f, -math.pi / 2, math.pi / 2, points=kinks or None, epsabs=1e-10, epsrel=1e-10, limit=400)
    return min(max(val, 0.0), 1.0)


def shutter_edge_coverage(pixel, half_plane, kind, r, shift):
    """An axis-aligned edge on an instance that translates during the shutter: the lit side is n . x >= c + shift * t, t
    uniform on [0, 1) (the K_TIME draw, tracer.rs:579-583; a translation interpolates linearly). The mean over t of the
    closed-form coverage: the box CDF convolved with a uniform density, by the CDF's integral."""
    nx, ny, c = half_plane
    if kind != "box" or (nx != 0.0 and ny != 0.0):
        raise ValueError("shutter_edge_coverage: a box filter and an axis-aligned edge")
    if shift == 0.0:
        return edge_coverage(pixel, half_plane, kind, r)
    n, at = (nx, pixel[0]) if ny == 0.0 else (ny, pixel[1])
    z0, z1 = c / n - at, (c + shift) / n - at
    mean_cdf = (_box_cdf_integral(r, z1) - _box_cdf_integral(r, z0)) / (z1 - z0)
    p = 1.0 - mean_cdf if n > 0.0 else mean_cdf
    return min(max(p, 0.0), 1.0)


# ---------------------------------------------------------------- the stopping rule ----------------------------------------------------------------
def relative_standard_error(n, k, L):
    """tracer.rs:609-617 on a two-valued pixel: after n samples, k of which saw luminance L and the rest 0,
        lum_sum = k L, lum_sq = k L^2,
        var_of_mean = (lum_sq - lum_sum^2 / n) / (n - 1) / n = L^2 k (n - k) / (n^2 (n - 1)),
        mean = max(k L / n, 1e-4),
    and the rule compares sqrt(var_of_mean) / mean with the threshold. Above the floor the L cancels:
        sqrt(k (n - k) / (n^2 (n - 1))) * n / k = sqrt((n - k) / (k (n - 1))).
    At or below it (k = 0 included, where the variance is 0): L sqrt(k (n - k) / (n - 1)) / n / 1e-4."""
    if k * L / n > 1e-4:
        return math.sqrt((n - k) / (k * (n - 1.0)))
    return L * math.sqrt(k * (n - k) / (n - 1.0)) / n / 1e-4


def stop_count(lit_sequence, L, min_spp, threshold, spp):
    """Samples the adaptive rule takes of a pixel whose s-th sample is lit (luminance L) or not (0). The rule is looked at
    after sample n for every n >= max(min_spp, 2) with n % 4 == 0 (tracer.rs:537, :609) and stops where the relative
    standard error is BELOW the threshold (a float32 setting, compared in float64); it never looks when threshold <= 0."""
    lit = np.asarray(lit_sequence, bool)
    threshold = float(np.float32(threshold))
    first = max(int(min_spp), 2)
    if threshold > 0.0:
        for n in range(4 * -(-first // 4), spp + 1, 4):
            if relative_standard_error(n, int(lit[:n].sum()), float(L)) < threshold:
                return n
    return spp


# ---------------------------------------------------------------- the module's own checks ----------------------------------------------------------------
def self_test():
    rng = np.random.default_rng(7)
    # the CDFs against a histogram-free check: derivative = pdf, ends 0 and 1, median at the centre
    for kind, r in (("box", 0.5), ("box", 1.25), ("triangle", 1.0), ("triangle", 2.0)):
        lo, hi = filter_support(kind, r)
        assert filter_cdf(kind, r, lo) == 0.0 and filter_cdf(kind, r, hi) == 1.0 and filter_cdf(kind, r, 0.5) == 0.5
        for x in rng.uniform(lo, hi, 20):
            h = 1e-6
            assert abs((filter_cdf(kind, r, x + h) - filter_cdf(kind, r, x - h)) / (2 * h) - filter_pdf(kind, r, x)) < 1e-5
        assert abs(integrate.quad(lambda x: filter_pdf(kind, r, x), lo, hi, points=[0.5])[0] - 1.0) < 1e-12
    # the generic slanted integral reproduces the polygon under the box of radius 0.5, and the axis-aligned closed form
    for _ in range(60):
        ang = rng.uniform(0, 2 * math.pi)
        n = (math.cos(ang), math.sin(ang))
        px = (int(rng.integers(0, 24)), int(rng.integers(0, 20)))
        c = n[0] * (px[0] + rng.uniform(-0.2, 1.2)) + n[1] * (px[1] + rng.uniform(-0.2, 1.2))
        assert abs(edge_coverage(px, (n[0], n[1], c)) - coverage_polygon(px, (n[0], n[1], c))) < 1e-10
    for hp, want in (((1.0, 0.0, 9.3), 0.7), ((-1.0, 0.0, -9.3), 0.3), ((0.0, 1.0, 7.6), 0.0), ((0.0, -1.0, -3.5), 0.5),
                     ((0.0, -1.0, -4.5), 1.0)):
        assert abs(coverage_polygon((9, 3), hp) - want) < 1e-12 and abs(edge_coverage((9, 3), hp) - want) < 1e-12
    # a wide filter's slanted integral against plain Monte Carlo of the inverse CDFs' offsets (filter.rs:196-204 restated)
    u = rng.random((400000, 2))
    tent = lambda u, r: 0.5 + np.where(u < 0.5, r * (np.sqrt(2 * u) - 1), r * (1 - np.sqrt(2 * (1 - u))))
    hp = (-0.347, 0.938, 3.1)
    hp = (hp[0] / math.hypot(hp[0], hp[1]), hp[1] / math.hypot(hp[0], hp[1]), hp[2])
    mc = np.mean(hp[0] * (5 + tent(u[:, 0], 1.5)) + hp[1] * (5 + tent(u[:, 1], 1.5)) >= hp[2])
    assert abs(edge_coverage((5, 5), hp, "triangle", 1.5) - mc) < 5 * 0.5 / math.sqrt(len(u))
    # the lens: d = f is the pinhole; the coverage does not depend on the blur's sign; a blur far wider than the pixel
    # gives the chord CDF at the pixel's centre
    for hp in ((1.0, 0.0, 9.3), (hp[0], hp[1], hp[2] + 5.0)):
        for px in ((9, 3), (8, 7), (10, 9)):
            assert lens_edge_coverage(px, hp, "box", 0.5, 0.0) == coverage_polygon(px, hp)
            assert abs(lens_edge_coverage(px, hp, "box", 0.5, 1e-9) - coverage_polygon(px, hp)) < 1e-7
            assert abs(lens_edge_coverage(px, hp, "box", 0.5, 1.7) - lens_edge_coverage(px, hp, "box", 0.5, -1.7)) < 1e-12
    a = (9.3 - 9.5) / 400.0  # lit where centre + 400 a' >= 9.3  <=>  a' >= a: 1 - chordCDF(a)
    chord_cdf = 0.5 + (a * math.sqrt(1 - a * a) + math.asin(a)) / math.pi
    assert abs(lens_edge_coverage((9, 3), (1.0, 0.0, 9.3), "box", 0.5, 400.0) - (1.0 - chord_cdf)) < 1e-6
    # the lens formula against rays: camera_ray's crossing of the plane at d, lens points uniform on the disc
    cam = dict(lookfrom=(0.9, 0.7, 1.1), lookat=(0.1, 0.2, 0.0), vup=(0.1, 1.0, 0.05), vfov_deg=40.0, aspect=1.2, aperture=0.3,
               focus_dist=1.4491376746189439)
    fr = camera_frame(cam)
    for d_rel in (0.6, 1.5):
        d = d_rel * fr["focus"]
        b = lens_blur(cam, 24, 20, d)
        x, y, lens = 7.3, 11.9, (0.31, -0.77)
        o, dirn = camera_ray(cam, x / 24, y / 20, lens)
        hit = o + dirn * ((-d - (o - fr["origin"]) @ fr["w"]) / (dirn @ fr["w"]))
        want = plane_point(cam, x + b * lens[0], y + b * lens[1], 24, 20, d)
        assert np.linalg.norm(hit - want) < 1e-12, (hit, want)
    # the shutter: against the mean over t of the static coverage
    for px in ((8, 2), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2)):
        want = integrate.quad(lambda t: edge_coverage(px, (1.0, 0.0, 9.3 + 3.0 * t)), 0, 1, epsabs=1e-12, limit=200)[0]
        assert abs(shutter_edge_coverage(px, (1.0, 0.0, 9.3), "box", 0.5, 3.0) - want) < 1e-9
        want = integrate.quad(lambda t: edge_coverage(px, (-1.0, 0.0, -9.3 - 3.0 * t)), 0, 1, epsabs=1e-12, limit=200)[0]
        assert abs(shutter_edge_coverage(px, (-1.0, 0.0, -9.3), "box", 0.5, -3.0) - want) < 1e-9
    # the stopping rule: the formula against the running sums in exact rational arithmetic
    from fractions import Fraction
    for n in (4, 8, 12, 64):
        for k in range(0, n + 1):
            for L in (Fraction(3, 100000), Fraction(47, 40)):
                s, q = k * L, k * L * L
                var = (q - s * s / n) / (n - 1) / n
                mean = max(s / n, Fraction(1, 10000))
                assert abs(relative_standard_error(n, k, float(L)) - math.sqrt(var) / float(mean)) < 1e-12
    lit = np.zeros(64, bool)
    assert [stop_count(lit, 1.0, m, t, 64) for m, t in ((1, 0.05), (5, 0.2), (8, 0.5), (16, 1e-6), (64, 10.0))] == [4, 8, 8, 16, 64]
    assert [stop_count(~lit, 1.0, m, t, 64) for m, t in ((1, 0.05), (5, 0.2), (8, 0.5), (16, 1e-6), (64, 10.0))] == [4, 8, 8, 16, 64]
    lit[::2] = True
    assert stop_count(lit, 1.0, 16, 1e-6, 64) == 64 and stop_count(lit, 1.0, 1, 0.0, 64) == 64
    assert stop_count(lit, 1.0, 8, 0.5, 64) == 8      # sqrt(4 / (4 * 7)) = 0.378
    assert stop_count(lit, 1.0, 1, 0.2, 64) == 28     # sqrt(1 / (n - 1)) < 0.2 from n = 27: the next multiple of 4
    assert stop_count(lit, 3e-5, 1, 0.05, 64) == 12   # under the floor: 0.3 * sqrt(n^2 / 4 / (n - 1)) / n = 0.15 / sqrt(n - 1)
    return True


if __name__ == "__main__":
    self_test()
    print("image_ref: self-test passed")
