"""Scenes and rays for the Tri4 packet step and the stored flat normals (tests/test_gpu_packet_step.py on the device,
tests/test_flat_normals.py on the host). Every scene is a SceneDesc, so one description serves the batched queries and
the renderer; `World.build_world` is usda.build_world with a mesh's shading normals passed on.

  masks    two interleaved meshes of 8 triangles each with different visibility masks (camera | indirect, shadow |
           indirect): every packet of the strip mixes them, so mask_and does not decide for camera and shadow rays.
  stack    four parallel triangles of shrinking size in one leaf (a ray along z crosses 4, 3, 2 or 1 of them), two
           exactly coincident triangles (the tie goes to the later lane), and triangles whose f32 normal is exactly
           zero in front of a valid plate (accepted by the edge test, refused for their normal).
  normals  a smooth-shaded and a flat sphere side by side, and the flat one again under a nested instance.
"""
import numpy as np

import fixtures as fx

f32 = np.float32
MASK_ALL = 0xFFFFFFFF
CAMERA, SHADOW, INDIRECT = 1, 2, 4
NAMES = ("masks", "stack", "normals")
STACK_SIZES = (8.0, 6.0, 4.0, 2.0)  # legs of the four parallel triangles at z = 0, 1, 2, 3
STACK_X = 10.0  # their right angle sits at (STACK_X, 0, z)


class World:
    """usda-module stand-in (build_world only): as usda.build_world, and a mesh's "normals" reach attach_triangles."""

    def __init__(self, usda):
        self.usda = usda

    def build_world(self, desc, api, new_material):
        protos = []
        for p in desc.protos:
            b = api.SceneBuilder()
            if "instances" in p:
                for it in p["instances"]:
                    b.attach_instance(protos[it["proto"]], it["l2w"], None, mask=it["mask"])
            else:
                b.attach_triangles(p["verts"], p["idx"], normals=p.get("normals"))
            protos.append(b.commit())
        b = api.SceneBuilder()
        materials = []
        for g in desc.geoms:
            if g["kind"] == "mesh":
                b.attach_triangles(g["verts"], g["idx"], normals=g.get("normals"), mask=g["mask"])
            else:
                b.attach_instance(protos[g["proto"]], g["l2w"], None, mask=g["mask"])
            materials.append(self.usda.fill_material(new_material(), g["material"]))
        return b.commit(), materials, protos


def _affine12(m3, t):
    m = np.asarray(m3, dtype=np.float32)
    return np.concatenate([m[:, 0], m[:, 1], m[:, 2], np.asarray(t, dtype=np.float32)]).astype(np.float32)


def _mesh(verts, idx, tint, mask=MASK_ALL, normals=None, name="mesh"):
    g = dict(kind="mesh", verts=np.asarray(verts, f32), idx=np.asarray(idx, np.uint32), mask=mask,
             material={"base_color": tint}, name=name)
    if normals is not None:
        g["normals"] = np.asarray(normals, f32)
    return g


def _finish(d, lookfrom, lookat, light_at, light_size, light_normal=(0, -1, 0)):
    """A rect light (invisible to shadow rays, as the importer makes them), the camera, 64 x 36 at depth 4."""
    o = np.asarray(light_at, f32)
    eu, ev = np.array([light_size, 0, 0], f32), np.array([0, 0, light_size], f32)
    if light_normal[2] != 0:
        ev = np.array([0, light_size, 0], f32)
    verts = np.stack([o, o + eu, o + eu + ev, o + ev]).astype(f32)
    rad = (12.0, 12.0, 12.0)
    d.geoms.append(dict(kind="mesh", verts=verts, idx=np.array([(0, 1, 2), (0, 2, 3)], np.uint32), mask=MASK_ALL & ~SHADOW,
                        material={"_preset": "emissive", "emission_color": rad}, name="light"))
    d.lights.append(dict(kind="rect", geom_id=len(d.geoms) - 1, radiance=np.array(rad, f32), origin=o, edge_u=eu, edge_v=ev,
                         normal=np.array(light_normal, f32)))
    d.camera = dict(lookfrom=np.asarray(lookfrom, f32), lookat=np.asarray(lookat, f32), vup=np.array([0, 1, 0], f32),
                    vfov_deg=f32(50), aspect=f32(64 / 36), aperture=f32(0), focus_dist=f32(6))
    d.settings.update(width=64, height=36, max_depth=4, spp=4)
    return d


def desc(usda, name):
    d = usda.SceneDesc()
    if name == "masks":
        # a strip of 16 triangles on y = 0: the even ones one mesh (camera | indirect), the odd ones the other (shadow |
        # indirect) — neighbours in space, so the builder packs them into the same Tri4 packets
        va, vb = [], []
        for k in range(16):
            (va if k % 2 == 0 else vb).extend([(k, 0, 0), (k, 0, 2), (k + 1, 0, 0)])
        ia = np.arange(24, dtype=np.uint32).reshape(8, 3)
        d.geoms.append(_mesh(va, ia, (0.8, 0.3, 0.2), CAMERA | INDIRECT, name="even"))
        d.geoms.append(_mesh(vb, ia, (0.2, 0.4, 0.8), SHADOW | INDIRECT, name="odd"))
        d.geoms.append(_mesh([(-4, -1, -4), (20, -1, -4), (20, -1, 6), (-4, -1, 6)], [(0, 2, 1), (0, 3, 2)], (0.7, 0.7, 0.7), name="floor"))
        return _finish(d, (8, 5, 9), (8, 0, 1), (6, 6, -1), 4.0)
    if name == "stack":
        v, i = [], []
        for z, s in enumerate(STACK_SIZES):
            i.append((len(v), len(v) + 1, len(v) + 2))
            v += [(STACK_X, 0, z), (STACK_X + s, 0, z), (STACK_X, s, z)]
        d.geoms.append(_mesh(v, i, (0.7, 0.6, 0.3), name="stack"))
        d.geoms.append(_mesh([(20, 0, 1), (22, 0, 1), (20, 2, 1)], [(0, 1, 2), (0, 1, 2)], (0.3, 0.7, 0.3), name="coincident"))
        # a sliver whose f32 cross product is exactly zero (Tri4::normal_ok = 0, prim.rs:81-83) although its area is not
        # (tests/edge_rays.py, "degenerate" 5), with a plate behind it
        sliver = [(0, 0, 0), (3, 1, 0), (3 + 2.0 ** -21, 1 + 2.0 ** -23, 0)]
        d.geoms.append(_mesh(sliver + [(-2, -2, 2), (6, -2, 2), (-2, 6, 2)], [(0, 1, 2), (3, 4, 5)], (0.5, 0.5, 0.8), name="zero normal"))
        d.geoms.append(_mesh([(-6, -6, 8), (40, -6, 8), (40, 12, 8), (-6, 12, 8)], [(0, 1, 2), (0, 2, 3)], (0.7, 0.7, 0.7), name="back"))
        return _finish(d, (12, 3, -16), (12, 2, 4), (8, 12, -4), 6.0)
    if name == "normals":
        v, i = fx.uv_sphere((-1.5, 1.0, 0.0), 1.0, 10, 5)
        n = v - np.array([-1.5, 1.0, 0.0], f32)
        n = (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)).astype(f32)
        d.geoms.append(_mesh(v, i, (0.8, 0.5, 0.3), normals=n, name="smooth"))
        v2, i2 = fx.uv_sphere((1.5, 1.0, 0.0), 1.0, 10, 5)
        d.geoms.append(_mesh(v2, i2, (0.3, 0.6, 0.8), name="flat"))
        v3, i3 = fx.uv_sphere((0.0, 0.0, 0.0), 1.0, 10, 5)
        d.protos.append(dict(verts=v3, idx=i3))
        rot = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]], f32)
        d.protos.append(dict(instances=[dict(proto=0, l2w=_affine12(rot * f32(0.75), (0.0, 0.25, 0.0)), mask=MASK_ALL)]))
        d.geoms.append(dict(kind="instance", proto=1, l2w=_affine12(np.diag([1.0, 1.5, 1.0]), (0.0, 1.2, -2.5)), mask=MASK_ALL,
                            material={"base_color": (0.4, 0.8, 0.4)}, name="nested flat"))
        d.geoms.append(_mesh([(-8, 0, -8), (8, 0, -8), (8, 0, 8), (-8, 0, 8)], [(0, 2, 1), (0, 3, 2)], (0.7, 0.7, 0.7), name="floor"))
        return _finish(d, (0, 2.5, 7), (0, 1, 0), (-2, 6, -2), 4.0)
    raise KeyError(name)


def _rays(o, d, mask):
    rays = np.zeros((len(o), 8), f32)
    rays[:, 0:3], rays[:, 3:6] = np.asarray(o, f32), np.asarray(d, f32)
    rays[:, 7] = np.full(len(o), mask, np.uint32).view(f32)
    return rays


def rays(name):
    """-> [(ray mask, rays[n, 8])]: `masks` 512 rays for each of the renderer's three ray masks, `stack` one batch of
    lattice rays from either side plus the tie and zero-normal rays, `normals` 1024 rays."""
    rng = np.random.default_rng({"masks": 5, "stack": 6, "normals": 7}[name])
    if name == "masks":
        out = []
        for m in (CAMERA, INDIRECT, SHADOW):
            tgt = np.stack([rng.uniform(-0.5, 16.5, 512), np.zeros(512), rng.uniform(-0.25, 2.25, 512)], axis=1)
            o = tgt + np.stack([rng.uniform(-3, 3, 512), rng.choice([-1.0, 1.0], 512) * rng.uniform(1, 4, 512), rng.uniform(-3, 3, 512)], axis=1)
            out.append((m, _rays(o, tgt - o, m)))
        return out
    if name == "stack":
        g = np.arange(-0.25, 8.5, 0.5)
        xy = np.stack(np.meshgrid(g + STACK_X, g), axis=-1).reshape(-1, 2)
        n = len(xy)
        o, d = [], []
        for z0, dz in ((-1.0, 1.0), (10.0, -1.0)):   # along z, from either side: 4, 3, 2, 1 or 0 triangles crossed
            o.append(np.column_stack([xy, np.full(n, z0)])); d.append(np.tile([0.0, 0.0, dz], (n, 1)))
            o.append(np.column_stack([xy, np.full(n, z0)])); d.append(np.tile([0.0625, -0.03125, dz], (n, 1)))  # slanted
        tie = np.array([(20.25 + 0.25 * (k % 5), 0.25 + 0.25 * (k // 5), -1.0) for k in range(15)])
        o += [tie, tie + (0, 0, 4.0)]; d += [np.tile([0.0, 0.0, 1.0], (15, 1)), np.tile([0.0, 0.0, -1.0], (15, 1))]
        # at the sliver: its vertices, points of its long edge (exact zeros of an edge function: the f64 fallback lanes)
        # and lattice points x with y = f32(x / 3), a third of which fall inside it
        xs = np.concatenate([[0.0, 3.0, 1.5, 0.75, 2.25], np.arange(1, 48) * 0.0625])
        zn = np.column_stack([xs, (xs.astype(f32) / f32(3.0)).astype(f32), np.full(len(xs), -1.0)])
        o += [zn, zn + (0, 0, 2.5)]; d += [np.tile([0.0, 0.0, 1.0], (len(zn), 1)), np.tile([0.0, 0.0, -1.0], (len(zn), 1))]
        return [(MASK_ALL, _rays(np.concatenate(o), np.concatenate(d), MASK_ALL))]
    tgt = np.concatenate([rng.normal(0, 0.6, (340, 3)) + (-1.5, 1.0, 0.0), rng.normal(0, 0.6, (340, 3)) + (1.5, 1.0, 0.0),
                          rng.normal(0, 0.6, (344, 3)) + (0.0, 1.5, -2.5)])
    o = tgt + rng.normal(0, 1, (1024, 3)) * 6.0
    return [(MASK_ALL, _rays(o, tgt - o, MASK_ALL))]


def stack_crossings(r):
    """How many of the four parallel triangles a ray along +-z crosses (exact for the lattice rays: none on an edge)."""
    x, y = r[:, 0].astype(np.float64) - STACK_X, r[:, 1].astype(np.float64)
    along_z = (r[:, 3] == 0) & (r[:, 4] == 0) & (x > -1) & (x < 9)
    n = sum(((x > 0) & (y > 0) & (x + y < s)).astype(int) for s in STACK_SIZES)
    return np.where(along_z, n, -1)


def flat_normal_f32(v9):
    """prim.rs:76-95 in float32, operation by operation: edges, cross product, sqrt of the dot product, divisions.
    v9: [n, 9] vertices -> [n, 3] (NaN / infinities for a zero cross product, as the arithmetic gives)."""
    v9 = np.asarray(v9, f32)
    e1, e2 = v9[:, 3:6] - v9[:, 0:3], v9[:, 6:9] - v9[:, 0:3]
    x = (e1[:, 1] * e2[:, 2]).astype(f32) - (e2[:, 1] * e1[:, 2]).astype(f32)
    y = (e1[:, 2] * e2[:, 0]).astype(f32) - (e2[:, 2] * e1[:, 0]).astype(f32)
    z = (e1[:, 0] * e2[:, 1]).astype(f32) - (e2[:, 0] * e1[:, 1]).astype(f32)
    with np.errstate(all="ignore"):
        ln = np.sqrt((((x * x).astype(f32) + (y * y).astype(f32)).astype(f32) + (z * z).astype(f32)).astype(f32)).astype(f32)
        return np.stack([(x / ln).astype(f32), (y / ln).astype(f32), (z / ln).astype(f32)], axis=1)
