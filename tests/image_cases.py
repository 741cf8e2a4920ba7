"""Tiny scenes whose every PIXEL has a known value, as SceneDesc builders (style of tests/radiometry_cases.py), and that
value from tests/image_ref.py. Used by tests/test_image_formation.py (the CPU oracle against the truth) and
tests/test_gpu_image_formation.py (the device against the oracle and against the truth).

A BACKDROP emissive quad of radiance (0.25, 0.5, 1.0) fills the frame; in front of it a CARD emissive quad of radiance
(2, 1, 0.5) faces the camera, perpendicular to the view axis, one edge of it crossing the frame. A sample is one of the two
colours, so a pixel's expectation is backdrop + (card - backdrop) * coverage, coverage being the closed form of
image_ref for the case's filter, lens and shutter. No lights, max_depth 1: an Emissive does not scatter (emissive.rs:30-38),
so the path ends at the first hit. (Depth 0 would end every path BEFORE its first intersection, tracer.rs:1123-1149: a
black frame. Depth 1 is also the least the camera launches ask for.) Every sum of up to 256 of these colours is exact in
float32, so a pixel the edge does not touch must hold its colour exactly.

Frame 24 x 20 (aspect 1.2, no multiple of 16: two tile columns and two tile rows), vfov 40, a camera whose axes have
no zero component; 256 spp, frames 0..3. The edge is given in camera-plane pixel coordinates (image_ref's half-plane)
and carried to the card's plane by image_ref's own float64 camera, so the scene does not depend on the camera under test.

`python tests/image_cases.py [case name prefixes]` measures every case on the CPU oracle at 16 x the tests' samples
(4 frames at 4096 spp) and prints the table MEASURED below was copied from."""
import ctypes as C
import importlib
import math
import os
import sys

import numpy as np

import image_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # run as a script: no conftest.py has put the package's parent on the path
    sys.path.insert(0, ROOT)
usda = importlib.import_module("crust-render_amd.usda")

W, H = 24, 20
SPP = 256
FRAMES = 4
MASK = 0xFFFFFFFF
BACKDROP = np.array([0.25, 0.5, 1.0])
CARD = np.array([2.0, 1.0, 0.5])
K_SIGMA = 5.0
# The error of an Owen-scrambled net's estimate has at most e times the variance of plain Monte Carlo with as many
# samples (Owen 1998, for (0, m, s)-nets in base 2 the constant is e = 2.718...): the binomial figure times sqrt(e) bounds
# the standard error without a look at the code under test.
OWEN = math.sqrt(math.e)
LOOKFROM, LOOKAT, VUP = (0.9, 0.7, 1.1), (0.1, 0.2, 0.0), (0.1, 1.0, 0.05)


# ---------------------------------------------------------------- pieces ----------------------------------------------------------------
def camera(width=W, height=H, vfov_deg=40.0, aperture=0.0):
    lookfrom, lookat = np.array(LOOKFROM, np.float32), np.array(LOOKAT, np.float32)
    return dict(lookfrom=lookfrom, lookat=lookat, vup=np.array(VUP, np.float32), vfov_deg=np.float32(vfov_deg),
                aspect=np.float32(width / height), aperture=np.float32(aperture),
                focus_dist=np.float32(np.linalg.norm(lookfrom - lookat)))


def settings(frame, kind, radius, width=W, height=H):
    return dict(usda.DEFAULTS, strategy="power", filter=kind, filter_radius=radius, width=width, height=height, max_depth=1,
                frame=frame, spp=SPP)


def emissive(rgb):
    return {"_preset": "emissive", "emission_color": tuple(float(x) for x in rgb)}


def quad(cam, corners_px, width, height, d):
    """Two triangles over four points given in pixel coordinates, on the plane at distance d along the view axis."""
    verts = np.array([ir.plane_point(cam, x, y, width, height, d) for x, y in corners_px], np.float32)
    return verts, np.array([(0, 1, 2), (0, 2, 3)], np.uint32)


def backdrop_geom(cam, width, height, rgb=BACKDROP):
    f = ir.camera_frame(cam)["focus"]
    v, i = quad(cam, [(-width, -height), (2 * width, -height), (2 * width, 2 * height), (-width, 2 * height)], width, height, 3.0 * f)
    return dict(kind="mesh", verts=v, idx=i, mask=MASK, material=emissive(rgb), name="backdrop")


def card_mesh(cam, half_plane, width, height, d):
    """The card: a quad of 6 frame widths on the lit side of the half-plane, its edge centred on the frame's centre."""
    nx, ny, c = half_plane
    cx, cy = width / 2.0, height / 2.0
    off = c - (nx * cx + ny * cy)
    ex, ey = cx + off * nx, cy + off * ny  # the point of the edge nearest the frame's centre
    tx, ty, L = -ny, nx, 3.0 * max(width, height)
    return quad(cam, [(ex - L * tx, ey - L * ty), (ex + L * tx, ey + L * ty), (ex + L * tx + L * nx, ey + L * ty + L * ny),
                      (ex - L * tx + L * nx, ey - L * ty + L * ny)], width, height, d)


def unit(nx, ny, through):
    """The half-plane with normal direction (nx, ny) whose edge passes through the pixel-coordinate point `through`."""
    n = math.hypot(nx, ny)
    nx, ny = nx / n, ny / n
    return (nx, ny, nx * through[0] + ny * through[1])


SLANTED = unit(-0.37, 1.0, (0.0, 5.27))      # y >= 5.27 + 0.37 x: from (0, 5.27) to (24, 14.15)
VERTICAL = unit(1.0, 0.0, (9.3, 0.0))        # x >= 9.3
HORIZONTAL = unit(0.0, 1.0, (0.0, 7.6))      # y >= 7.6
DIAGONAL = unit(1.0, 1.0, (12.2, 10.1))      # x + y >= 22.3: 45 degrees, where a square lens differs most from a disc
STRIP_EDGE = unit(1.0, 0.0, (257.4, 0.0))    # past the 256-pixel tile-domain boundary (tracer.rs:543)


class Case:
    """name; build(frame) -> SceneDesc; coverage() -> [height, width] float64 in buffer order (row j, column i)."""

    def __init__(self, name, half_plane, kind="box", radius=0.5, d_rel=0.8, aperture=0.0, motion_px=0.0, width=W, height=H,
                 vfov_deg=40.0, card=CARD, backdrop=BACKDROP):
        self.name, self.half_plane, self.kind, self.radius, self.d_rel = name, half_plane, kind, radius, d_rel
        self.aperture, self.motion_px, self.width, self.height = aperture, motion_px, width, height
        self.card, self.backdrop = np.asarray(card, np.float64), np.asarray(backdrop, np.float64)
        self.cam = camera(width, height, vfov_deg, aperture)
        self.pinhole = aperture == 0.0 and motion_px == 0.0
        self._coverage = None

    def build(self, frame):
        d = usda.SceneDesc()
        cam, w, h = self.cam, self.width, self.height
        d.geoms.append(backdrop_geom(cam, w, h, self.backdrop))
        if self.half_plane is not None:
            dist = self.d_rel * ir.camera_frame(cam)["focus"]
            verts, idx = card_mesh(cam, self.half_plane, w, h, dist)
            if self.motion_px:  # an instance whose end transform is a translation along +u (usda.py, crust:motion:translate)
                move = ir.plane_point(cam, self.motion_px, 0.0, w, h, dist) - ir.plane_point(cam, 0.0, 0.0, w, h, dist)
                d.protos.append(dict(verts=verts, idx=idx))
                d.geoms.append(dict(kind="instance", proto=0, l2w=usda.affine12(usda._m4()),
                                    l2w_end=usda.affine12(usda._translation(move)), mask=MASK, material=emissive(self.card),
                                    name="card"))
            else:
                d.geoms.append(dict(kind="mesh", verts=verts, idx=idx, mask=MASK, material=emissive(self.card), name="card"))
        d.camera, d.settings = cam, settings(frame, self.kind, self.radius, w, h)
        return d

    def coverage(self):
        if self._coverage is None:
            cov = np.zeros((self.height, self.width))
            if self.half_plane is not None:
                nx, ny, c = self.half_plane
                dist = self.d_rel * ir.camera_frame(self.cam)["focus"]
                blur = ir.lens_blur(self.cam, self.width, self.height, dist) if self.aperture else 0.0
                for j in range(self.height):
                    for i in range(self.width):
                        if self.motion_px:  # the card's lit side n . (x - m t) >= c
                            cov[j, i] = ir.shutter_edge_coverage((i, j), self.half_plane, self.kind, self.radius, nx * self.motion_px)
                        elif self.aperture:
                            cov[j, i] = ir.lens_edge_coverage((i, j), self.half_plane, self.kind, self.radius, blur)
                        elif (self.kind, self.radius) == ("box", 0.5):
                            cov[j, i] = ir.coverage_polygon((i, j), self.half_plane)
                        else:
                            cov[j, i] = ir.edge_coverage((i, j), self.half_plane, self.kind, self.radius)
            self._coverage = cov
        return self._coverage

    def truth(self):
        return self.backdrop + (self.card - self.backdrop) * self.coverage()[..., None]

    def allowance(self):
        """Bias allowance as a fraction of card - backdrop: twice the deviation measured for this case, at most 2e-3."""
        return min(2.0 * abs(MEASURED[self.name][0]), MAX_ALLOWANCE)


FILTERS = (("box", 0.5), ("box", 1.25), ("triangle", 1.0), ("triangle", 2.0))


def cases():
    out = [Case("pinhole_slanted", SLANTED)]
    for kind, r in FILTERS:
        out.append(Case("pinhole_vertical_%s%g" % (kind, r), VERTICAL, kind, r))
        out.append(Case("pinhole_horizontal_%s%g" % (kind, r), HORIZONTAL, kind, r))
    out.append(Case("triangle_slanted", SLANTED, "triangle", 1.5))
    out.append(Case("lens_defocus_vertical", VERTICAL, d_rel=0.6, aperture=0.3))
    out.append(Case("lens_defocus_horizontal", HORIZONTAL, d_rel=0.6, aperture=0.3))
    out.append(Case("lens_defocus_diagonal", DIAGONAL, d_rel=0.6, aperture=0.3))
    out.append(Case("lens_defocus_behind", DIAGONAL, d_rel=1.5, aperture=0.3))  # 1 - d/f < 0: the blur disc mirrored
    out.append(Case("lens_in_focus", SLANTED, d_rel=1.0, aperture=0.3))
    out.append(Case("lens_flat_field", None, "triangle", 1.5, aperture=0.3))
    out.append(Case("shutter_edge", VERTICAL, motion_px=3.0))
    out.append(Case("wide_strip", STRIP_EDGE, width=260, height=2, vfov_deg=0.5))
    return out


def stop_case(card_luminance=None):
    """pinhole_slanted over a BLACK backdrop (an Emissive of colour 0: it ends the path as the lit one does), for the
    stopping rule: a sample's luminance is the card's or 0. card_luminance: a grey card of that luminance instead."""
    card = CARD if card_luminance is None else np.full(3, card_luminance)
    return Case("stop_slanted" if card_luminance is None else "stop_slanted_%g" % card_luminance, SLANTED, card=card,
                backdrop=np.zeros(3))


def luminance(rgb):
    """guiding/mod.rs:18-20 in float32, as render_pixel applies it to a sample's colour."""
    r, g, b = (np.float32(x) for x in rgb)
    return float(np.float32(np.float32(np.float32(0.2126) * r + np.float32(0.7152) * g) + np.float32(0.0722) * b))


# ---------------------------------------------------------------- rendering and the bound ----------------------------------------------------------------
def oracle_render(desc, spp):
    import ora_world
    return ora_world.OracleRenderer(desc, usda).render(spp, forward=1)[0]


def mean_image(render, case, frames=FRAMES, spp=SPP):
    """render(desc, spp) -> image [height, width, 3]. -> the float64 mean of the frames' images (`frame` seeds sampler_new)."""
    return np.mean([np.asarray(render(case.build(f), spp), np.float64) for f in range(frames)], axis=0)


def violations(case, mean, n_samples, allowance):
    """The pixels, rows and columns of a mean image that break the bound -> list of (what, index, got, truth, bound).
    Per pixel and channel: |mean - truth| <= (K sqrt(e) sqrt(p (1 - p) / N) + allowance) * |card - backdrop|, N the
    samples behind the mean, p the true coverage; where p is 0 or 1 the pixel must EQUAL its colour. Row and column sums:
    the same with sum p (1 - p) under the root (the pixels' samples are independent draws of different pixels; the
    variances add) and the allowance once per pixel the edge touches."""
    p = case.coverage()
    truth = case.truth()
    contrast = np.abs(case.card - case.backdrop)
    var = p * (1.0 - p) / n_samples
    mixed = (p > 0.0) & (p < 1.0)
    bad = []
    bound = (K_SIGMA * OWEN * np.sqrt(var) + allowance * mixed)[..., None] * contrast
    err = np.abs(mean - truth)
    for j, i in np.argwhere(np.any((err > bound) | (~mixed[..., None] & (mean != truth)), axis=2)):
        bad.append(("pixel", (int(i), int(j)), mean[j, i], truth[j, i], bound[j, i]))
    for axis, what in ((1, "row"), (0, "column")):
        b = (K_SIGMA * OWEN * np.sqrt(var.sum(axis=axis)) + allowance * mixed.sum(axis=axis))[:, None] * contrast
        got, want = mean.sum(axis=axis), truth.sum(axis=axis)
        for k in np.argwhere(np.any(np.abs(got - want) > b + 1e-12 * np.abs(want), axis=1))[:, 0]:
            bad.append((what, int(k), got[k], want[k], b[k]))
    return bad


def deviation(case, mean):
    """Largest |mean - truth| over pixels and channels as a fraction of |card - backdrop|."""
    if case.half_plane is None:
        return float(np.abs(mean - case.truth()).max())
    return float((np.abs(mean - case.truth()) / np.abs(case.card - case.backdrop)).max())


def oracle_samples(case, spp, frame=0):
    """[height, width, spp, 3] float32: every sample's colour by ora_render_sample (camera_sample + trace_path)."""
    import ora
    import ora_world
    o = ora_world.OracleRenderer(case.build(frame), usda)
    out = np.zeros((case.height, case.width, spp, 3), np.float32)
    rgb, st = np.zeros(3, np.float32), ora.RayStats()
    for j in range(case.height):
        for i in range(case.width):
            for s in range(spp):
                ora.lib().ora_render_sample(C.byref(o.job), i, j, s, ora._fp(rgb), C.byref(st))
                out[j, i, s] = rgb
    return out


def oracle_adaptive(case, spp, min_spp, threshold, frame=0):
    """-> (counts [height, width] uint32, image [height, width, 3] float32) of render_pixel under the stopping rule."""
    import ora
    import ora_world
    o = ora_world.OracleRenderer(case.build(frame), usda, variance=threshold, min_spp=min_spp)
    o.job.spp = spp
    counts, img = np.zeros((case.height, case.width), np.uint32), np.zeros((case.height, case.width, 3), np.float32)
    rgb, st = np.zeros(3, np.float32), ora.RayStats()
    for j in range(case.height):
        for i in range(case.width):
            counts[j, i] = ora.lib().ora_render_pixel(C.byref(o.job), i, j, ora._fp(rgb), C.byref(st))
            img[j, i] = rgb
    return counts, img


def sequential_mean(samples, counts):
    """The float32 sum of each pixel's first counts[j, i] sample colours in sample order, divided by that count."""
    h, w, spp, _ = samples.shape
    total = np.zeros((h, w, 3), np.float32)
    for s in range(spp):
        total = np.where((s < counts)[..., None], total + samples[:, :, s], total).astype(np.float32)
    return (total / counts.astype(np.float32)[..., None]).astype(np.float32)


STOP_RULES = ((1, 0.05), (5, 0.2), (8, 0.5), (16, 1e-6), (64, 10.0))
STOP_SPP = 64
STOP_FIRST_CHECK = (4, 8, 8, 16, 64)


def expected_counts(case, samples, min_spp, threshold, spp=STOP_SPP):
    """image_ref.stop_count of every pixel's lit sequence; asserts that every sample is exactly the card or the backdrop."""
    card, back = case.card.astype(np.float32), case.backdrop.astype(np.float32)
    lit = np.all(samples == card, axis=-1)
    assert np.all(lit | np.all(samples == back, axis=-1)), "a sample that is neither the card's colour nor the backdrop's"
    L = luminance(card)
    return np.array([[ir.stop_count(lit[j, i], L, min_spp, threshold, spp) for i in range(case.width)] for j in range(case.height)],
                    np.uint32), lit


def check_stop_shape(counts, lit, min_spp, threshold, bright):
    """What the counts must look like whatever the sequences are: a pixel whose samples up to the first look at the rule
    are all lit or all dark stops there (4, 8, 8, 16, 64 for STOP_RULES); at 1e-6 a pixel that is mixed by then takes
    every sample; the middle rules tell mixed pixels apart."""
    first = STOP_FIRST_CHECK[STOP_RULES.index((min_spp, threshold))]
    head = lit[..., :first]
    flat = head.all(axis=-1) | ~head.any(axis=-1)
    assert flat.any() and (~flat).any() and np.all(counts[flat] == first)
    assert np.all(counts % 4 == 0) and counts.min() >= first and counts.max() <= STOP_SPP
    if threshold == 1e-6:
        assert np.all(counts[~flat] == STOP_SPP)
    if bright and (min_spp, threshold) in ((5, 0.2), (8, 0.5)):  # at 0.05 a mixed pixel of 64 samples hardly ever stops
        assert len(np.unique(counts[~flat])) > 2


# Bias allowance, as a fraction of card - backdrop: what float32 camera and intersection arithmetic can move the edge by.
# A displaced edge adds the same sign of coverage to every pixel it crosses, so the measure is the MEAN SIGNED coverage
# error over the pixels on the edge (noise averages out of it, a displacement does not). MEASURED ON THE CPU ORACLE ONLY:
# 4 frames at 4096 spp (16 x the tests' samples) against image_ref; a test allows twice the measured figure per pixel, and
# never more than MAX_ALLOWANCE, the ceiling of the radiometry tests.
# name: (mean signed coverage error over the pixels on the edge, the largest pixel error as a share of K sqrt(e) SE at that N)
MAX_ALLOWANCE = 2e-3
MEASURED_BY = "python tests/image_cases.py"
MEASURED = {
    "pinhole_slanted": (+9.7e-05, 0.06),  # 33 pixels on the edge; the others exact: True
    "pinhole_vertical_box0.5": (-9.2e-06, 0.00),  # 20 pixels on the edge; the others exact: True
    "pinhole_horizontal_box0.5": (+1.5e-06, 0.00),  # 24 pixels on the edge; the others exact: True
    "pinhole_vertical_box1.25": (+6.9e-06, 0.01),  # 60 pixels on the edge; the others exact: True
    "pinhole_horizontal_box1.25": (-7.7e-06, 0.01),  # 72 pixels on the edge; the others exact: True
    "pinhole_vertical_triangle1": (+9.2e-06, 0.01),  # 40 pixels on the edge; the others exact: True
    "pinhole_horizontal_triangle1": (+2.0e-06, 0.03),  # 48 pixels on the edge; the others exact: True
    "pinhole_vertical_triangle2": (-6.1e-06, 0.03),  # 80 pixels on the edge; the others exact: True
    "pinhole_horizontal_triangle2": (+2.9e-06, 0.07),  # 96 pixels on the edge; the others exact: True
    "triangle_slanted": (+5.0e-05, 0.35),  # 99 pixels on the edge; the others exact: True
    "lens_defocus_vertical": (-4.2e-05, 0.13),  # 100 pixels on the edge; the others exact: True
    "lens_defocus_horizontal": (-1.4e-05, 0.15),  # 120 pixels on the edge; the others exact: True
    "lens_defocus_diagonal": (-1.1e-04, 0.18),  # 138 pixels on the edge; the others exact: True
    "lens_defocus_behind": (+5.6e-05, 0.10),  # 100 pixels on the edge; the others exact: True
    "lens_in_focus": (+9.7e-05, 0.06),  # 33 pixels on the edge; the others exact: True
    "lens_flat_field": (+0.0e+00, 0.00),  # 0 pixels on the edge; the others exact: True
    "shutter_edge": (+6.0e-05, 0.40),  # 80 pixels on the edge; the others exact: True
    "wide_strip": (-2.4e-05, 0.00),  # 2 pixels on the edge; the others exact: True
}


if __name__ == "__main__":
    only = sys.argv[1:]
    for c in cases():
        if only and not any(c.name.startswith(o) for o in only):
            continue
        n = FRAMES * 16 * SPP
        mean = mean_image(oracle_render, c, FRAMES, 16 * SPP)
        p = c.coverage()
        mixed = (p > 0.0) & (p < 1.0)
        exact = bool(np.all(mean[~mixed] == c.truth()[~mixed]))
        bias, share = 0.0, 0.0
        if mixed.any():
            rel = (mean - c.truth()) / (c.card - c.backdrop)  # the coverage the image shows minus the true one, per channel
            bias = float(rel[mixed].mean())
            share = float((np.abs(rel[mixed]) / (K_SIGMA * OWEN * np.sqrt(p * (1.0 - p) / n))[mixed][:, None]).max())
        print('    "%s": (%+.1e, %.2f),  # %d pixels on the edge; the others exact: %s' % (c.name, bias, share, int(mixed.sum()), exact),
              flush=True)
