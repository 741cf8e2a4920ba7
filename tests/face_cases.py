"""Seeded inputs for the per-face texture tests (test infrastructure), shared by tests/test_face_textures.py (CPU) and
tests/test_gpu_face_textures.py: textures from 1x1 to 64x16 texels, face maps with all four slices, bindings in both swap
states, hit records and coordinates that include the exact edges. Everything is authored as the Python lists
tests/face_ref.py takes; `aggregate` hands the same lists to the library."""
import numpy as np

import face_ref as fr
import seam_cases as sc

f32, u32 = np.float32, np.uint32
HIT = np.dtype([("t", f32), ("normal", f32, 3), ("front_face", u32), ("u", f32), ("v", f32), ("geom_id", u32), ("prim_id", u32),
                ("_pad", u32)])
COORD = np.dtype([("face_id", u32), ("u", f32), ("v", f32), ("_pad", u32)])
assert HIT.itemsize == 40 and COORD.itemsize == 16
MISS = 0xFFFFFFFF

# per face (width, height): 1x1 up to 64x16, both orientations, two faces without texels, one that is no power of two
SIZES = [(1, 1), (2, 1), (1, 2), (4, 4), (64, 16), (16, 64), (8, 2), (0, 4), (4, 0), (32, 32), (3, 5), (2, 2)]


def texture(rng, sizes=SIZES):
    """(sizes, texels [n, 3]) with every texel distinct and in [0, 1)."""
    n = sum(w * h for w, h in sizes)
    return list(sizes), rng.uniform(0.0, 1.0, size=(n, 3)).astype(f32)


def edge_values(rng, n):
    """n coordinates: uniform in [0, 1), with exact 0, exact 1, -0.0 and values just outside mixed in."""
    x = rng.uniform(0.0, 1.0, size=n).astype(f32)
    pick = rng.integers(0, 16, size=n)
    x[pick == 0] = 0.0
    x[pick == 1] = 1.0
    x[pick == 2] = -0.0
    x[pick == 3] = np.nextafter(f32(1.0), f32(0.0))
    return x


def eval_queries(rng, n, sizes, refusals=True):
    """COORD records over a texture of `sizes`: every face, texel centres, the edges; with `refusals` also a face id past
    the table, NO_FACE, NaN and infinite coordinates and coordinates outside [0, 1]."""
    q = np.zeros(n, COORD)
    q["face_id"] = rng.integers(0, len(sizes), size=n)
    q["u"], q["v"] = edge_values(rng, n), edge_values(rng, n)
    wh = np.asarray(sizes, np.int64)[q["face_id"]]
    centre = (rng.integers(0, 4, size=n) == 0) & (wh[:, 0] > 0) & (wh[:, 1] > 0)
    w, h = np.maximum(wh[:, 0], 1), np.maximum(wh[:, 1], 1)
    i, j = rng.integers(0, 1 << 30, size=n) % w, rng.integers(0, 1 << 30, size=n) % h
    q["u"][centre] = ((i + 0.5) / w).astype(f32)[centre]
    q["v"][centre] = ((j + 0.5) / h).astype(f32)[centre]
    if refusals:
        pick = rng.integers(0, 64, size=n)
        q["face_id"][pick == 0] = len(sizes) + rng.integers(0, 1000, size=int((pick == 0).sum()))
        q["face_id"][pick == 1] = fr.NO_FACE
        q["u"][pick == 2] = np.nan
        q["v"][pick == 3] = np.inf
        q["u"][pick == 4] = -np.inf
        q["v"][pick == 5] = np.nan
        q["u"][pick == 6] = rng.uniform(-3.0, 0.0, size=int((pick == 6).sum())).astype(f32)
        q["v"][pick == 7] = rng.uniform(1.0, 4.0, size=int((pick == 7).sum())).astype(f32)
    return q


def face_maps(rng, n_faces):
    """Three maps [(faces, slices)]: quads only, a mix of all four slices, triangles only; face ids below n_faces + 3 (a
    few name a face the texture does not have)."""
    out = []
    quads = rng.integers(0, n_faces, size=40).astype(u32)
    out.append((np.repeat(quads, 2), np.tile(np.array([fr.QUAD_LOWER, fr.QUAD_UPPER], np.uint8), 40)))
    out.append((rng.integers(0, n_faces + 3, size=61).astype(u32), rng.integers(0, 4, size=61).astype(np.uint8)))
    out.append((rng.integers(0, n_faces, size=17).astype(u32), np.zeros(17, np.uint8)))
    return out


# geom_id -> (map, swapped): both swap states of every map; geometries 1, 4 and everything from 8 on are unbound
BINDINGS = {0: (0, False), 2: (0, True), 3: (1, False), 5: (1, True), 6: (2, False), 7: (2, True)}


def hits(rng, n, maps, bindings=BINDINGS):
    """HIT records: bound and unbound geometries, misses, prim ids up to a few past each map, barycentrics with the exact
    corners and edges."""
    h = np.zeros(n, HIT)
    h["geom_id"] = rng.integers(0, 11, size=n)
    h["geom_id"][rng.integers(0, 8, size=n) == 0] = MISS
    longest = max(len(m[0]) for m in maps)
    h["prim_id"] = rng.integers(0, longest + 4, size=n)
    for g, (m, _) in bindings.items():  # most prim ids inside the geometry's own map
        sel = np.nonzero((h["geom_id"] == g) & (rng.integers(0, 8, size=n) != 0))[0]
        h["prim_id"][sel] = rng.integers(0, len(maps[m][0]), size=len(sel))
    u = edge_values(rng, n)
    v = (edge_values(rng, n) * (f32(1.0) - np.abs(u))).astype(f32)
    corner = rng.integers(0, 16, size=n)
    u[corner == 0], v[corner == 0] = 1.0, 0.0
    u[corner == 1], v[corner == 1] = 0.0, 1.0
    u[corner == 2], v[corner == 2] = 0.75, 0.75  # u + v = 1.5: only the clamp keeps a quad's coordinate inside
    h["u"], h["v"] = u, v
    h["t"] = rng.uniform(0.1, 10.0, size=n).astype(f32)
    h["normal"] = (0.0, 0.0, 1.0)
    h["front_face"] = 1
    return h


def aggregate(crt, textures, maps=(), bindings=None, material_texture=()):
    """crt.textures.FaceTextures from the authored lists: textures [(sizes, texels)] or [(sizes, texels, fallback)]."""
    T = crt.textures
    tex = [T.FaceTexture(t[0], t[1], t[2] if len(t) > 2 else (0.5, 0.5, 0.5)) for t in textures]
    bind = [(g, m, s) for g, (m, s) in (bindings or {}).items()]
    return T.FaceTextures(tex, [T.FaceMap(f, s) for f, s in maps], bind, material_texture)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(u32)


def textured_case(crt, cls, n, seed):
    """-> (ft, mats, q, coords, substituted per-query table, its queries): materials of one lobe class, every third one
    untextured, two textures; coordinates with NO_FACE mixed in."""
    rng = np.random.default_rng(seed)
    mats = sc.materials(cls, 67, rng)
    tex_a, tex_b = texture(rng), texture(rng, [(4, 4), (1, 1), (16, 8)])
    material_texture = [None if i % 3 == 2 else i % 2 for i in range(len(mats))]
    ft = aggregate(crt, [tex_a, tex_b], material_texture=material_texture)
    q = sc.shade_queries(n, len(mats), rng)
    which = np.array([-1 if t is None else t for t in material_texture])[q["material"]]
    coords = np.zeros(n, COORD)
    for t, tex in enumerate((tex_a, tex_b)):
        sel = np.nonzero(which == t)[0]
        coords[sel] = eval_queries(rng, len(sel), tex[0], refusals=False)
    sel = np.nonzero(which < 0)[0]
    coords[sel] = eval_queries(rng, len(sel), tex_a[0], refusals=False)
    coords["face_id"][rng.integers(0, 8, size=n) == 0] = fr.NO_FACE
    # the truth: one material per query, base_color = face_ref's texel where the query is textured
    table = mats[q["material"]].copy()
    for t, tex in enumerate((tex_a, tex_b)):
        sel = np.nonzero((which == t) & (coords["face_id"] != fr.NO_FACE))[0]
        table["base_color"][sel] = fr.texture_eval(tex[0], tex[1], (0.5, 0.5, 0.5), coords["face_id"][sel], coords["u"][sel], coords["v"][sel])
    q_sub = q.copy()
    q_sub["material"] = np.arange(n, dtype=u32)
    textured = (which >= 0) & (coords["face_id"] != fr.NO_FACE)
    return ft, mats, q, coords, table, q_sub, textured
