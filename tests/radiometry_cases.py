"""Tiny scenes with a known pixel value, as SceneDesc builders (style of tests/test_infinite_lights.py:_world), and the
value of each from tests/radiometry_ref.py. Used by tests/test_radiometry.py (the CPU oracle against the truth) and
tests/test_gpu_radiometry.py (the device against the oracle and against the truth).

Frame: 16 x 16, box filter of radius 0.5, pinhole, a narrow field of view. Under the box filter the 256 pixels tile the
frame, so the mean over the pixels estimates the mean of the pixel expectation E(s, t) over the frame square; the truth
is that mean by a 3 x 3 Gauss-Legendre rule over (s, t), E being smooth across so narrow a frame.

Material: OpenPBR, base_weight 1, specular_weight 0, base_diffuse_roughness 0, grey base_color: Lambert times
1 - F0 plus the residual Schlick lobe that specular_weight 0 leaves (radiometry_ref.slab_f, DESIGN.md "Radiometry").

A scene that must not see the sky gradient carries a black uniform dome (tracer.rs:1000-1008); the dome is also one
more light in NEE's pick, so the 1/n_lights factor is exercised.

`python tests/radiometry_cases.py [case name prefixes]` measures every case's bias on the CPU oracle (16 frames at
1024 spp, 16 x the tests' samples) and prints the table MEASURED below was copied from. Strategies left out: `bsdf` for
the DistantLight at 0 and 2 degrees (a delta-like light); every other case runs all four."""
import importlib
import os
import sys

import numpy as np

import radiometry_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # run as a script: no conftest.py has put the package's parent on the path
    sys.path.insert(0, ROOT)
usda =importlib.import_module("crust-render_amd.usda")

W = H = 16
SPP = 64
FRAMES = 16
ALL = ("power", "balance", "light", "bsdf")
MASK = 0xFFFFFFFF
RHO = 0.5


# ---------------------------------------------------------------- pieces ----------------------------------------------------------------
def slab(roughness, ior, rho=RHO, emission=0.0):
    m = {"base_color": (rho, rho, rho), "base_weight": 1.0, "specular_weight": 0.0, "base_diffuse_roughness": 0.0,
         "specular_roughness": roughness, "specular_ior": ior}
    if emission:
        m.update(emission_luminance=1.0, emission_color=(emission, emission, emission))
    return m


def camera(lookfrom, lookat, vfov_deg):
    lookfrom, lookat = np.array(lookfrom, np.float32), np.array(lookat, np.float32)
    return dict(lookfrom=lookfrom, lookat=lookat, vup=np.array([0, 1, 0], np.float32), vfov_deg=np.float32(vfov_deg),
                aspect=np.float32(1.0), aperture=np.float32(0), focus_dist=np.float32(np.linalg.norm(lookfrom - lookat)))


def camera_ray(cam, s, t):
    """camera.rs:27-63 in float64: the pinhole ray through frame position (s, t) in [0,1]^2 -> (origin, unit direction)."""
    o, at, up = (np.asarray(cam[k], np.float64) for k in ("lookfrom", "lookat", "vup"))
    w = (o - at) / np.linalg.norm(o - at)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    half = np.tan(np.radians(float(cam["vfov_deg"])) / 2.0)
    focus = float(cam["focus_dist"])
    horizontal, vertical = u * (focus * 2.0 * half * float(cam["aspect"])), v * (focus * 2.0 * half)
    d = (o - horizontal / 2 - vertical / 2 - w * focus) + s * horizontal + t * vertical - o
    return o, d / np.linalg.norm(d)


def frame_mean(cam, pixel_expectation):
    """Mean over the frame of pixel_expectation(origin, direction) by a 3 x 3 Gauss-Legendre rule."""
    x, wt = np.polynomial.legendre.leggauss(3)
    x, wt = (x + 1) / 2, wt / 2
    return sum(wi * wj * np.asarray(pixel_expectation(*camera_ray(cam, si, tj)), np.float64)
               for si, wi in zip(x, wt) for tj, wj in zip(x, wt))


def settings(strategy, frame, depth):
    return dict(usda.DEFAULTS, strategy=strategy, filter="box", filter_radius=0.5, width=W, height=H, max_depth=depth,
                frame=frame, spp=SPP)


def ground(material):
    g = np.array([(-50, 0, -50), (50, 0, -50), (50, 0, 50), (-50, 0, 50)], dtype=np.float32)
    return dict(kind="mesh", verts=g, idx=np.array([(0, 2, 1), (0, 3, 2)], np.uint32), mask=MASK, material=material,
                name="ground")


def ground_hit(o, d):
    """Where a camera ray meets the plane y = 0, and the view vector in the hit frame (x, -z, y): z is the normal."""
    p = o - d * (o[1] / d[1])
    return p, to_hit_frame(-d)


def to_hit_frame(a):
    a = np.asarray(a, np.float64)
    return np.array([a[0], -a[2], a[1]])


def black_dome():
    return usda.dome_light((0.0, 0.0, 0.0))


def rect_light(desc, origin, edge_u, edge_v, normal, radiance):
    o, eu, ev = (np.asarray(a, np.float32) for a in (origin, edge_u, edge_v))
    n = np.asarray(normal, np.float64)
    verts = np.stack([o, o + eu, o + eu + ev, o + ev]).astype(np.float32)
    rad = np.full(3, radiance, np.float32)
    desc.geoms.append(dict(kind="mesh", verts=verts, idx=np.array([(0, 1, 2), (0, 2, 3)], np.uint32), mask=MASK,
                           material={"_preset": "emissive", "emission_color": tuple(rad)}, name="rect"))
    desc.lights.append(dict(kind="rect", geom_id=len(desc.geoms) - 1, radiance=rad, origin=o, edge_u=eu, edge_v=ev,
                            normal=(n / np.linalg.norm(n)).astype(np.float32)))


def sphere_light(desc, center, radius, radiance):
    c, rad = np.asarray(center, np.float32), np.full(3, radiance, np.float32)
    desc.geoms.append(dict(kind="sphere", center=c, radius=np.float32(radius), mask=MASK,
                           material={"_preset": "emissive", "emission_color": tuple(rad)}, name="lamp"))
    desc.lights.append(dict(kind="sphere", geom_id=len(desc.geoms) - 1, radiance=rad, center=c, radius=np.float32(radius)))


class Case:
    """name; build(strategy, frame) -> SceneDesc; truth() -> RGB mean of the frame; the strategies it runs under and, where
    one is left out, why."""

    def __init__(self, name, build, truth, strategies=ALL, left_out=None):
        self.name, self._build, self._truth, self.strategies, self.left_out = name, build, truth, strategies, left_out
        self._value = None
        assert len(ALL) - len(strategies) <= 1 and (left_out is not None) == (len(strategies) < len(ALL))

    def build(self, strategy, frame):
        return self._build(strategy, frame)

    def truth(self):
        if self._value is None:
            self._value = np.broadcast_to(np.asarray(self._truth(), np.float64), (3,)).copy()
        return self._value

    def allowance(self, strategy):
        """Bias allowance as a fraction of the truth: twice the deviation measured for this case and strategy, at most 2e-3."""
        m = MEASURED[self.name]
        return min(2.0 * abs(m.get(strategy, m.get("all"))[0]), MAX_ALLOWANCE)


# ---------------------------------------------------------------- the cases ----------------------------------------------------------------
PLANE_CAM = camera((0, 4, 3), (0, 0, 0), 1.0)
PLANE_ROUGH, PLANE_IOR = 0.3, 1.5
DOME_RADIANCE = np.array([1.0, 0.7, 0.4])


def furnace(ior):
    """A convex sphere under a uniform dome, depth 4: every bounce escapes, the pixel is radiance * albedo(view). The
    dome is the only light. All four strategies."""
    cam = camera((0, 0, 8), (0, 0, 0), 4.0)
    rough = 0.3

    def build(strategy, frame):
        d = usda.SceneDesc()
        d.geoms.append(dict(kind="sphere", center=np.zeros(3, np.float32), radius=np.float32(1.0), mask=MASK,
                            material=slab(rough, ior), name="ball"))
        d.lights.append(usda.dome_light(tuple(DOME_RADIANCE)))
        d.camera, d.settings = cam, settings(strategy, frame, 4)
        return d

    def pixel(o, d):
        b = o @ d
        p = o + d * (-b - np.sqrt(b * b - (o @ o - 1.0)))
        return DOME_RADIANCE * rr.albedo(-(d @ p), RHO, ior, rough)

    return Case("furnace_ior%.1f" % ior, build, lambda: frame_mean(cam, pixel))


SUN_TRAVEL = np.array([0.3, -1.0, 0.2])
SUN_IRRADIANCE = 2.0


def plane_scene(strategy, frame, lights, depth=2):
    d = usda.SceneDesc()
    d.geoms.append(ground(slab(PLANE_ROUGH, PLANE_IOR)))
    lights(d)
    d.lights.append(black_dome())
    d.camera, d.settings = PLANE_CAM, settings(strategy, frame, depth)
    return d


def sun_pixel(angle_deg, travel=SUN_TRAVEL):
    to_light = to_hit_frame(-travel / np.linalg.norm(travel))

    def pixel(o, d):
        _p, v = ground_hit(o, d)
        if angle_deg == 0.0:
            return rr.distant_zero_angle(v, to_light, SUN_IRRADIANCE, RHO, PLANE_IOR, PLANE_ROUGH)
        return rr.distant_cone(v, to_light, np.radians(angle_deg) / 2.0, SUN_IRRADIANCE, RHO, PLANE_IOR, PLANE_ROUGH)
    return pixel


def distant(angle_deg):
    """The plane under a DistantLight whose cone has the given full angle (0: DistantLight::new clamps it to 0.05 degrees,
    light.rs:255-266, a cone 4e-4 rad wide whose quadrature is the centre-direction formula to 1e-7). Depth 2: the bounce
    ray carries the other half of the MIS weight and escapes into the black dome. `bsdf` is left out at 0 and 2 degrees:
    a cone of 1e-3 sr or less is a delta-like light, found by a cosine-distributed bounce a few times per frame."""
    sun = lambda d: d.lights.append(usda.distant_light(SUN_TRAVEL, (SUN_IRRADIANCE,) * 3, angle_deg))
    narrow = angle_deg <= 2.0
    return Case("distant_%gdeg" % angle_deg, lambda s, f: plane_scene(s, f, sun), lambda: frame_mean(PLANE_CAM, sun_pixel(angle_deg)),
                ALL[:3] if narrow else ALL, "bsdf: delta-like light" if narrow else None)


def _strip():
    n = np.array([0.5, -1.0, 0.0]) / np.linalg.norm([0.5, -1.0, 0.0])
    eu = np.cross(n, [0.0, 0.0, 1.0])
    eu = 2.0 * eu / np.linalg.norm(eu)
    ev = 0.5 * np.cross(n, eu / 2.0)
    centre = np.array([1.5, 1.5, -0.5])
    return centre - eu / 2 - ev / 2, eu, ev, n


RECTS = {"square": ((-0.2, 2.0, -0.7), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0), 6.0),  # overhead, facing down
         "strip": _strip() + (12.0,)}  # 2 x 0.5, 72 degrees between its normal and the direction to the shading point


def rect_pixel(which):
    o_, eu, ev, n, radiance = RECTS[which]
    # what the oracle integrates is the float32 rectangle the scene holds
    o32, eu32, ev32 = (np.asarray(a, np.float32).astype(np.float64) for a in (o_, eu, ev))

    def pixel(o, d):
        p, v = ground_hit(o, d)
        return rr.rect_light(v, to_hit_frame(o32 - p), to_hit_frame(eu32), to_hit_frame(ev32), to_hit_frame(n), radiance,
                             RHO, PLANE_IOR, PLANE_ROUGH)
    return pixel


def rect(which):
    """The plane under a one-sided RectLight that faces it. All four strategies: a bounce ray finds the rectangle."""
    lamp = lambda d: rect_light(d, *RECTS[which])
    return Case("rect_" + which, lambda s, f: plane_scene(s, f, lamp), lambda: frame_mean(PLANE_CAM, rect_pixel(which)))


SPHERES = {"far": ((0.5, 3.0, 0.3), 0.3, 20.0),
           "near": ((0.8, 0.1, 0.0), 0.3, 5.0)}  # 22 degree cap whose centre stands 7 degrees over the horizon: cut by it


def sphere_pixel(which):
    c, r, radiance = SPHERES[which]
    c32, r32 = np.asarray(c, np.float32).astype(np.float64), float(np.float32(r))

    def pixel(o, d):
        p, v = ground_hit(o, d)
        return rr.sphere_light(v, to_hit_frame(c32 - p), r32, radiance, RHO, PLANE_IOR, PLANE_ROUGH)
    return pixel


def sphere(which):
    """The plane under a SphereLight. All four strategies."""
    lamp = lambda d: sphere_light(d, *SPHERES[which])
    return Case("sphere_" + which, lambda s, f: plane_scene(s, f, lamp), lambda: frame_mean(PLANE_CAM, sphere_pixel(which)))


def two_lights():
    """The square RectLight and a 20 degree DistantLight together (three lights with the black dome): the sum of the two.
    The sun stands where the rectangle does not cover any of its cone (under SUN_TRAVEL the rectangle's edge shades 2 % of
    the cone, and the sum is 1.7e-4 too bright for the scene). All four strategies."""
    travel = np.array([0.6, -1.0, -0.8])

    def lamps(d):
        rect_light(d, *RECTS["square"])
        d.lights.append(usda.distant_light(travel, (SUN_IRRADIANCE,) * 3, 20.0))
    a, b = rect_pixel("square"), sun_pixel(20.0, travel)
    return Case("rect_and_distant", lambda s, f: plane_scene(s, f, lamps), lambda: frame_mean(PLANE_CAM, lambda o, d: a(o, d) + b(o, d)))


INTERIOR_R, INTERIOR_IOR, INTERIOR_LE = 3.0, 1.5, 1.0
INTERIOR_CAM = camera((1.2, 0.5, 0.4), (1.2, 0.5, -1.0), 10.0)  # off the centre: the first hit is oblique (cosine 0.9)
INTERIOR_DEPTHS, INTERIOR_ROUGH = (1, 2, 3, 6, 12), (0.05, 0.3, 1.0)


def interior(depth, rough, mesh=False):
    """Camera inside an emissive sphere that also scatters, no lights: L_depth of radiometry_ref.emissive_sphere_interior
    at the cosine of the first hit. With no light to pick, the four strategies run the same estimator; all four run.
    mesh: the shell as 40 x 20 flat triangles (fixtures.uv_sphere). A closed shell of any shape keeps the Lambert part of
    the series exactly; the facets turn the normals by up to 4.5 degrees, which moves only the residual lobe's part, and
    the mesh case runs at specular_roughness 1.0 where that part is 2e-4 of the pixel in all."""
    def build(strategy, frame):
        d = usda.SceneDesc()
        mat = slab(rough, INTERIOR_IOR, emission=INTERIOR_LE)
        if mesh:
            import fixtures
            v, i = fixtures.uv_sphere((0, 0, 0), INTERIOR_R, 40, 20)
            d.geoms.append(dict(kind="mesh", verts=v, idx=i, mask=MASK, material=mat, name="shell"))
        else:
            d.geoms.append(dict(kind="sphere", center=np.zeros(3, np.float32), radius=np.float32(INTERIOR_R), mask=MASK,
                                material=mat, name="shell"))
        d.camera, d.settings = INTERIOR_CAM, settings(strategy, frame, depth)
        return d

    def pixel(o, d):
        b = o @ d
        p = o + d * (-b + np.sqrt(b * b - (o @ o - INTERIOR_R ** 2)))
        return rr.emissive_sphere_interior(depth, INTERIOR_LE, (d @ p) / INTERIOR_R, RHO, INTERIOR_IOR, rough)

    return Case("interior%s_d%d_r%g" % ("_mesh" if mesh else "", depth, rough), build, lambda: frame_mean(INTERIOR_CAM, pixel))


def cases():
    out = [furnace(1.0), furnace(1.5), distant(0.0), distant(2.0), distant(20.0), rect("square"), rect("strip"),
           sphere("far"), sphere("near"), two_lights()]
    out += [interior(d, r) for r in INTERIOR_ROUGH for d in INTERIOR_DEPTHS]
    out.append(interior(3, 1.0, mesh=True))
    return out


# ---------------------------------------------------------------- rendering and the bound ----------------------------------------------------------------
def frame_means(render, case, strategy, frames, spp=SPP):
    """render(desc, spp) -> image [H, W, 3]. -> [frames, 3] float64: the mean over the pixels of each frame's image.
    `frame` seeds sampler_new, so the estimates are independent."""
    return np.array([np.asarray(render(case.build(strategy, f), spp), np.float64).mean(axis=(0, 1)) for f in range(frames)])


def oracle_render(desc, spp):
    import ora_world
    return ora_world.OracleRenderer(desc, usda).render(spp, forward=1)[0]


def mean_and_se(fm):
    return fm.mean(axis=0), fm.std(axis=0, ddof=1) / np.sqrt(len(fm))


# Bias allowance, as a fraction of the truth: what the estimator's named epsilons take or add. They are pdf.max(1e-4), the
# light pdf's .max(1e-6), cosine * area + 1e-4 (light.rs:180-187: an area light's NEE is 1e-4 / (cosine * area) too
# bright, 1.0e-4 for the square, 1.8e-4 = 2e-4 / area for the sphere lights), the 1e-4 origin offset, t_min, and the
# 1e-6 in the denominators of both MIS heuristics (the weights of one direction sum to 1 - 1e-6 / (a^2 + b^2): -1.9e-5
# under the dome). MEASURED ON THE CPU ORACLE ONLY: 16 frames at 1024 spp (16 x the tests' samples) against
# radiometry_ref, per case and strategy; a test allows twice the measured deviation, and never more than MAX_ALLOWANCE
# (sphere_far / bsdf, whose 2 x 1.1e-3 +- 1.6e-3 is noise, is held to the cap). Without a light to pick the four
# strategies are one computation, measured once ("all").
# name: {strategy: (measured relative deviation, its standard error)}
MAX_ALLOWANCE = 2e-3
MEASURED_ON, MEASURED_BY = "2026-10-20", "python tests/radiometry_cases.py"
MEASURED = {
    "furnace_ior1.0": {"power": (-1.9e-05, 5e-06), "balance": (-5.0e-07, 6e-06), "light": (+1.9e-05, 2e-05), "bsdf": (-5.8e-07, 4e-06)},  # truth 0.3333381
    "furnace_ior1.5": {"power": (-1.8e-05, 5e-06), "balance": (-1.4e-07, 6e-06), "light": (+1.9e-05, 2e-05), "bsdf": (-2.3e-07, 4e-06)},  # truth 0.3200048
    "distant_0deg": {"power": (+2.1e-07, 5e-09), "balance": (-2.2e-07, 5e-09), "light": (+2.1e-07, 5e-09)},  # truth 0.2704242
    "distant_2deg": {"power": (+6.8e-08, 5e-08), "balance": (+1.1e-05, 1e-05), "light": (+6.1e-08, 4e-08)},  # truth 0.2703857
    "distant_20deg": {"power": (+3.0e-06, 2e-06), "balance": (+5.1e-05, 4e-05), "light": (+2.4e-07, 4e-07), "bsdf": (+9.9e-04, 7e-04)},  # truth 0.2666044
    "rect_square": {"power": (+1.1e-04, 8e-06), "balance": (+1.3e-04, 6e-05), "light": (+1.0e-04, 1e-06), "bsdf": (+4.0e-04, 5e-04)},  # truth 0.19387
    "rect_strip": {"power": (+2.4e-04, 2e-05), "balance": (+2.6e-04, 1e-04), "light": (+2.5e-04, 7e-06), "bsdf": (+3.8e-04, 1e-03)},  # truth 0.09145086
    "sphere_far": {"power": (+1.8e-04, 2e-05), "balance": (+1.9e-04, 7e-05), "light": (+1.8e-04, 2e-05), "bsdf": (+1.1e-03, 2e-03)},  # truth 0.08890177
    "sphere_near": {"power": (+3.8e-04, 1e-04), "balance": (+4.2e-04, 2e-04), "light": (+3.3e-04, 6e-05), "bsdf": (-5.6e-05, 9e-04)},  # truth 0.01531733
    "rect_and_distant": {"power": (+6.2e-05, 1e-05), "balance": (+6.9e-05, 6e-05), "light": (+5.8e-05, 1e-05), "bsdf": (+6.1e-06, 6e-04)},  # truth 0.3455041
    "interior_d1_r0.05": {"all": (+2.05e-07, 1.2e-06)},  # truth 1.320009
    "interior_d2_r0.05": {"all": (+3.97e-05, 9.9e-05)},  # truth 1.424315
    "interior_d3_r0.05": {"all": (+1.55e-05, 1.3e-04)},  # truth 1.458367
    "interior_d6_r0.05": {"all": (-8.93e-06, 1.6e-04)},  # truth 1.474301
    "interior_d12_r0.05": {"all": (-1.61e-05, 1.6e-04)},  # truth 1.474875
    "interior_d1_r0.3": {"all": (-2.86e-07, 8.1e-07)},  # truth 1.320042
    "interior_d2_r0.3": {"all": (-9.96e-07, 1.2e-05)},  # truth 1.424079
    "interior_d3_r0.3": {"all": (+9.18e-06, 1.3e-05)},  # truth 1.457933
    "interior_d6_r0.3": {"all": (-1.20e-05, 2.8e-05)},  # truth 1.473702
    "interior_d12_r0.3": {"all": (+1.32e-07, 3.1e-05)},  # truth 1.474264
    "interior_d1_r1": {"all": (+9.07e-07, 1.1e-06)},  # truth 1.320043
    "interior_d2_r1": {"all": (-5.39e-06, 4.9e-06)},  # truth 1.422602
    "interior_d3_r1": {"all": (-5.83e-06, 5.9e-06)},  # truth 1.455467
    "interior_d6_r1": {"all": (-1.94e-05, 2.9e-05)},  # truth 1.470456
    "interior_d12_r1": {"all": (-2.40e-05, 3.0e-05)},  # truth 1.470965
    "interior_mesh_d3_r1": {"all": (+2.37e-06, 5.9e-06)},  # truth 1.455467
}


if __name__ == "__main__":
    only = sys.argv[1:]
    for c in cases():
        if only and not any(c.name.startswith(o) for o in only):
            continue
        lit = bool(c.build("power", 0).lights)
        rows = []
        for s in c.strategies if lit else c.strategies[:1]:
            m, se = mean_and_se(frame_means(oracle_render, c, s, FRAMES, 16 * SPP))
            rows.append((s if lit else "all", (m[0] - c.truth()[0]) / c.truth()[0], se[0] / c.truth()[0]))
        print('    "%s": {%s},  # truth %.7g' % (c.name, ", ".join('"%s": (%+.1e, %.0e)' % r for r in rows), c.truth()[0]), flush=True)
