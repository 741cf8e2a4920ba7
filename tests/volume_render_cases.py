"""Cases for volume renders, shared by tests/test_volume_render.py (the restatement on the CPU) and
tests/test_gpu_volume_render.py (the wavefront renderer against it): a scene description, the region dicts bound to it,
and the render settings. The smallest frames at which every arm of the volume-forward form is reached:
40 x 24 pixels, 4 samples, one batch unless a case says otherwise."""
import os

import numpy as np

import volume_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
f32 = np.float32


def scene_file(name):
    for d in (GOLDEN, os.path.join(ROOT, "scenes")):
        p = os.path.join(d, name + ".usda")
        if os.path.exists(p):
            return p
    raise FileNotFoundError(name)


def at_lookat(desc, regions, scale=1.0):
    """The regions moved (and scaled about their own origin) so that their origin sits on the camera's lookat point."""
    c = np.asarray(desc.camera["lookat"], f32)
    out = []
    for r in regions:
        m = np.asarray(r["local_to_world"] if r.get("local_to_world") is not None else [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32).copy()
        m[:9] *= f32(scale)
        m[9:12] = m[9:12] * f32(scale) + c
        out.append(dict(r, local_to_world=m))
    return out


def view_distance(desc):
    return float(np.linalg.norm(np.asarray(desc.camera["lookat"], f32) - np.asarray(desc.camera["lookfrom"], f32)))


def far_away(V):
    """An aggregate no ray of any test scene crosses."""
    return [V.region(local_to_world=vc.affine(translate=(4.0e4, 3.0e4, -5.0e4)), half_extent=1.0, sigma_s=1.0, sigma_a=0.5)]


class Case:
    def __init__(self, name, desc, regions, spp=4, depth=8, strategy=None, variance=0.0, min_spp=None, batch=None, mapped_dome=False):
        self.name, self.desc, self.regions, self.spp, self.depth = name, desc, regions, spp, depth
        self.variance, self.min_spp, self.batch, self.mapped_dome = variance, min_spp, batch, mapped_dome
        if strategy is not None:
            desc.settings["strategy"] = strategy


def _load(crt, name, w=40, h=24, **kw):
    return crt.usda.load(scene_file(name), w, h, **kw)


def _own_regions(crt, desc):
    keys = set(crt.volumes.region())
    return [{k: v for k, v in r.items() if k in keys} for r in desc.volumes]


# name -> builder(crt) -> Case: the cases of the GPU volume tests.
def _fog(depth, strategy=None):
    def make(crt):
        desc = _load(crt, "fog", volumes=True)
        return Case("fog", desc, _own_regions(crt, desc), depth=depth, strategy=strategy)
    return make


def _smoke(adaptive=False, w=40, h=24, spp=4):
    def make(crt):
        desc = _load(crt, "smoke", w, h, volumes=True)
        if adaptive:  # variance 0.05, min 4, budget 16, batches of 4
            return Case("smoke", desc, _own_regions(crt, desc), spp=16, depth=16, variance=0.05, min_spp=4, batch=4)
        return Case("smoke", desc, _own_regions(crt, desc), spp=spp, depth=16)
    return make


def _veach_nested(crt):
    desc = _load(crt, "veach_mis")
    return Case("veach_mis", desc, at_lookat(desc, vc.aggregates(crt.volumes)["nested_eight"], 0.2 * view_distance(desc)))


def _one_region(scene, depth=8, **kw):
    def make(crt):
        desc = _load(crt, scene)
        d = view_distance(desc)
        reg = dict(half_extent=0.3 * d, sigma_s=(1.2 / d, 0.9 / d, 0.7 / d), sigma_a=0.3 / d, g=0.4, emission=(0.3, 0.1, 0.05))
        reg.update(kw)
        return Case(scene, desc, at_lookat(desc, [crt.volumes.region(**reg)]), depth=depth)
    return make


def _showcase_in_fog(crt):
    """Carried media and regions together: every sphere of the showcase inside one homogeneous fog that also holds the
    camera."""
    desc = _load(crt, "openpbr_showcase")
    d = view_distance(desc)
    reg = crt.volumes.region(half_extent=3.0 * d, sigma_s=0.25 / d, sigma_a=0.05 / d, g=0.2)
    return Case("openpbr_showcase", desc, at_lookat(desc, [reg]), depth=12)


def _domelight_mapped(crt):
    desc = _load(crt, "domelight", environment_maps=True)
    d = view_distance(desc)
    reg = crt.volumes.region(half_extent=0.3 * d, sigma_s=1.0 / d, sigma_a=0.2 / d, g=-0.3)
    return Case("domelight", desc, at_lookat(desc, [reg]), mapped_dome=True)


CASES = {
    "fog_depth8_power": _fog(8, "power"),
    "fog_depth8_bsdf": _fog(8, "bsdf"),
    "fog_depth1": _fog(1),
    "fog_depth2": _fog(2),
    "smoke_depth16": _smoke(),
    "smoke_adaptive": _smoke(adaptive=True),
    "veach_mis_nested_eight": _veach_nested,
    "sun_sky_region": _one_region("sun_sky"),
    "openpbr_showcase_in_fog": _showcase_in_fog,
    "domelight_mapped_region": _domelight_mapped,
    "motionblur_region": _one_region("motionblur", depth=4, field="noise", noise_threshold=0.1, density_scale=3.0),
    "cornellbox_region": _one_region("cornellbox"),
}
COVERAGE = ("phase_vertices", "phase_nee", "depth_walks", "medium_walks", "phase_prev_hits", "phase_prev_escapes")
