"""Cases for guided renders, shared by tests/test_guided_render.py (the restatement tests/guided_pt on the CPU) and
tests/test_gpu_guided_render.py (the wavefront renderer against it): a scene description, the training passes of the field
bound to it, and the render settings. 24 x 16 pixels x 16 samples at depth 8 unless a case says otherwise.

Every field is built over the scene's bounds (crt_scene_bounds) from seeded synthetic samples — numpy default_rng,
positions uniform in the bounds, directions toward points of the scene's first area light (or the emissive panel, or into
a cone where the scene has neither), 2 to 3 updates. These fields exercise every arm of the guided pass; only STAT_CASES'
`cornell_bsdf` is also a GOOD field (see there). Nothing here renders: whoever needs the field builds it twice from
the same passes, once behind the ABI (crt.guiding.GuidingField: host code, no device) and, for the independent table,
once as the numpy restatement (guiding_ref.Field)."""
import os

import numpy as np

import guiding_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
f32 = np.float32
SEED = 20261021
# "It helps" (test_guided_render.py): the ratio guided / unguided of the mean per-pixel variance over 16 frames x 64 spp of
# `cornell_bsdf`, measured on the restatement with SEED above: 0.876 (0.87 to 0.90 with two and a half times the samples
# per pass and half or twice the leaves). The test asserts below sqrt(0.876 * 1) = 0.936. The gain is bounded: primary
# vertices are never guided (tracer.rs:1386) and their light hits carry most of the per-pixel variance.
MEASURED_VARIANCE_RATIO = 0.876


def scene_file(name):
    for d in (GOLDEN, os.path.join(ROOT, "scenes")):
        p = os.path.join(d, name + ".usda")
        if os.path.exists(p):
            return p
    raise FileNotFoundError(name)


def light_points(desc, rng, n):
    """n points on the scene's first area light (rect: uniform in the parallelogram; sphere: uniform on the surface)."""
    for l in desc.lights:
        if l["kind"] == "rect":
            uv = rng.uniform(size=(n, 2))
            return (np.asarray(l["origin"], np.float64) + uv[:, :1] * np.asarray(l["edge_u"], np.float64)
                    + uv[:, 1:] * np.asarray(l["edge_v"], np.float64))
        if l["kind"] == "sphere":
            d = rng.normal(size=(n, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            return np.asarray(l["center"], np.float64) + float(l["radius"]) * d
    return None


def toward(pos, points):
    d = points - pos
    return (d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)).astype(f32)


def cone(rng, n, axis=(0.3, 1.0, 0.2), spread=0.15):
    a = np.asarray(axis, np.float64)
    d = a / np.linalg.norm(a) + spread * rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def make_passes(desc, bounds, seed, n=4000, updates=3, target=None, where=None, spread=None, box=None, growth=1, presplit=0):
    """[(SAMPLE records, next_iteration)]. box: positions uniform in this box instead of the bounds. where: (centre, sigma)
    — a field trained in some leaves only, as guiding_cases' deep_spatial and zero_flux are: the first pass is uniform and
    carries no flux (counted, so the spatial tree splits into untrained leaves; never splat), the later ones cluster."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(bounds[:3], np.float64), np.asarray(bounds[3:], np.float64)
    if box is not None:
        lo, hi = np.asarray(box[:3], np.float64), np.asarray(box[3:], np.float64)
    passes = []
    if where is not None or presplit:
        m = presplit or n
        s = np.zeros(m, gr.SAMPLE)
        s["pos"], s["dir"] = rng.uniform(lo, hi, size=(m, 3)).astype(f32), cone(rng, m)
        passes.append((s, 1))
    n0 = n
    for k in range(len(passes), updates):
        n = n0 * growth ** k  # growth > 1: later passes outweigh the early ones, which were recorded in coarser leaves
        if where is None:
            pos = rng.uniform(lo, hi, size=(n, 3))
        else:
            pos = np.asarray(where[0], np.float64) + where[1] * rng.normal(size=(n, 3))
        pts = target(rng, n) if target is not None else light_points(desc, rng, n)
        direction = toward(pos, pts) if pts is not None else cone(rng, n)
        if spread:
            direction = direction + spread * rng.normal(size=(n, 3))
            direction = (direction / np.linalg.norm(direction, axis=1, keepdims=True))
        s = np.zeros(n, gr.SAMPLE)
        s["pos"], s["dir"], s["radiance"] = pos.astype(f32), direction.astype(f32), rng.uniform(0.5, 2.0, n).astype(f32)
        passes.append((s, k + 1))
    return passes


class Case:
    def __init__(self, name, scene, w=24, h=16, spp=16, depth=8, strategy=None, variance=0.0, min_spp=None, batch=None,
                 mapped_dome=False, cfg=None, passes=None, env=None, load=None, looks=None):
        self.name, self.scene, self.w, self.h, self.spp, self.depth = name, scene, w, h, spp, depth
        self.strategy, self.variance, self.min_spp, self.batch, self.mapped_dome = strategy, variance, min_spp, batch, mapped_dome
        self.cfg = dict(spatial_c=300.0, guide_prob=0.5)
        self.cfg.update(cfg or {})
        self.passes_kw = passes if passes is not None else {}
        self.env = env or {}          # environment knobs of the device renderer (CRT_SIMPLE=0: the general instances)
        self.load = load or {}        # keyword arguments of usda.load
        self.looks = looks or {}      # geometry name -> material fields laid over the file's (tests/test_gpu_environment.py's way)

    def desc(self, crt):
        if callable(self.scene):  # a scene built in code
            d = self.scene(crt)
            d.settings.update(width=self.w, height=self.h)
            d.camera["aspect"] = f32(self.w / self.h)
        else:
            d = crt.usda.load(scene_file(self.scene), self.w, self.h, **self.load)
        for g in d.geoms:
            if g["name"] in self.looks:
                g["material"] = dict(g["material"], **self.looks[g["name"]])
        assert sum(g["name"] in self.looks for g in d.geoms) == len(self.looks)
        if self.strategy is not None:
            d.settings["strategy"] = self.strategy
        return d

    def passes(self, desc, bounds):
        if self.passes_kw is False:  # an untrained field: one empty pass
            return [(np.zeros(0, gr.SAMPLE), 1)]
        return make_passes(desc, bounds, SEED + sum(map(ord, self.name)), **self.passes_kw)


def slab_scene(crt):
    """(c) media_cases' chromatic scattering slab made rough (continuous transmission: make_ray's medium flag) in front of
    the white wall, closed by the black shell, with media_cases' rect light of radiance 0 (the lit instances, shadow rays)."""
    import media_cases as mc
    mat = mc.glass(mc.SCATTER_TINT, 1.0, mc.SCATTER, 0.3, specular_roughness=0.5)
    d = mc.usda.SceneDesc()
    d.geoms += [mc.mesh(*mc.slab_mesh(), mat, "slab"), mc.wall()]
    return mc.finish(d, mc.camera((1.5, 1.0, 5.0), (0, 0, 0), 40.0), "power", 0, 8, form="rect")


def wall_points(rng, n):  # the white wall behind the slab
    return np.stack([rng.uniform(-4, 4, n), rng.uniform(-4, 4, n), np.full(n, -0.6)], axis=1)


def panel_points(rng, n):  # the emissive panel of cornellbox_emitter: the ceiling's middle
    return np.stack([rng.uniform(-0.5, 0.5, n), np.full(n, 3.99), rng.uniform(-0.5, 0.5, n)], axis=1)


def sun_points(rng, n):  # far along the distant light's direction reversed: a parallel beam
    return np.tile(np.array([[430.0, 740.0, 510.0]]), (n, 1))


_ROOM = "fog"  # tests/golden/fog.usda without its region: a Lambert room, a small rect light under the ceiling; simple materials
CASES = {
    # (a) the room under all four strategies, depth 32 so that roulette runs on guided throughput: the simple instances
    "room_power": Case("room_power", _ROOM, depth=32, strategy="power"),
    "room_balance": Case("room_balance", _ROOM, depth=32, strategy="balance"),
    "room_light": Case("room_light", _ROOM, depth=32, strategy="light"),
    "room_bsdf": Case("room_bsdf", _ROOM, depth=32, strategy="bsdf"),
    # ... and through the general instances (MATS 1): CRT_SIMPLE=0 makes the renderer class a simple table as general
    # (render.cpp, knobs.simple; tests/test_gpu_environment.py runs its `general_by_knob` case the same way). pipeline() does not report the
    # material class, so no test can assert that the MATS 1 instance ran: were the knob ignored, this case would repeat
    # room_power at depth 8. room_coat below is a general table in its own right; showcase and slab hold interior media.
    "room_general": Case("room_general", _ROOM, strategy="power", env={"CRT_SIMPLE": "0"}),
    # ... and MATS 1 for certain: a coat and fuzz on the room's walls and the ball make the table general, without a medium
    "room_coat": Case("room_coat", _ROOM, strategy="power",
                      looks=dict(Room=dict(coat_weight=0.8, coat_roughness=0.1, coat_color=(0.9, 0.8, 0.7), fuzz_weight=0.4, fuzz_roughness=0.5),
                                 Ball=dict(thin_film_weight=1.0, thin_film_thickness=0.45))),
    # (b), (c) the showcase's material classes: coat, fuzz, thin film, smooth and rough transmission, interior media (MATS 2)
    "showcase": Case("showcase", "openpbr_showcase", depth=8, cfg=dict(spatial_c=100.0)),
    "slab": Case("slab", slab_scene, passes=dict(target=wall_points, box=(-6, -6, -1, 6, 6, 6))),
    # (d) distant light and uniform dome (INF 1)
    "dome_uniform": Case("dome_uniform", "domelight", passes=dict(target=sun_points)),
    "sun_sky": Case("sun_sky", "sun_sky"),
    # (e) mapped dome (INF 2)
    "dome_mapped": Case("dome_mapped", "domelight", mapped_dome=True, load=dict(environment_maps=True), passes=dict(target=sun_points)),
    # (f) trained in some leaves and not in others: clustered samples and a low split threshold
    "room_partial": Case("room_partial", _ROOM, strategy="power", cfg=dict(spatial_c=4.0),
                         passes=dict(n=1500, updates=3, where=((-1.2, 0.6, -0.8), 0.35))),
    # (g) unlit room with an emissive panel (LIT false)
    "emitter": Case("emitter", "cornellbox_emitter", passes=dict(target=panel_points)),
    # (h) a moving instance
    "motionblur": Case("motionblur", "motionblur"),
    # (i) adaptive stopping: variance 0.05, min 4, budget 16, batches of 4
    "room_adaptive": Case("room_adaptive", _ROOM, strategy="power", variance=0.05, min_spp=4, batch=4),
    # (j) a partial wave
    "room_tiny": Case("room_tiny", _ROOM, w=5, h=3, spp=3, strategy="power"),
    # (k) an untrained field
    "room_untrained": Case("room_untrained", _ROOM, strategy="power", passes=False),
}
# The closed room the feature is for (scenes/cornellbox_guided.usda: a small sphere light under the ceiling): the statistics
# of tests/test_guided_render.py only, on the CPU.
STAT_CASES = {
    # (d) under every strategy: the guided bounce's mixture pdf against lights at infinity (escaped_emission)
    **{"dome_" + st: Case("dome_" + st, "domelight", strategy=st, passes=dict(target=sun_points)) for st in ("power", "balance", "light", "bsdf")},
    **{"sunsky_" + st: Case("sunsky_" + st, "sun_sky", strategy=st) for st in ("power", "balance", "light", "bsdf")},
    "cornell_power": Case("cornell_power", "cornellbox_guided", strategy="power"),
    # An INFORMED field. A spatial leaf that splits hands each child the parent's whole D-tree, sums undivided
    # (sdtree.rs:107-168), so flux recorded while the leaves were coarse outweighs what their children record later: the
    # fields above, whose first pass falls into one leaf, stay close to uniform (1 % of their draws reach the light) and
    # RAISE the variance (ratio 1.19 here). This one splits first — a pass of flux-free samples, counted and never splat —
    # and trains the 512 leaves with the two passes that follow: 6 to 20 % of its draws reach the light.
    "cornell_bsdf": Case("cornell_bsdf", "cornellbox_guided", strategy="bsdf", cfg=dict(spatial_c=100.0),
                         passes=dict(n=40000, presplit=40000)),
}
