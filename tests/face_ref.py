"""The truth for per-face textures (test infrastructure): FaceMap::resolve behind World::intersect's binding lookup
(crates/crust-core/src/rt_world.rs:64-77, :207-232) and PtexTexture::eval as the reference's renderer implements it
(crates/crust-render/src/main.rs:277-314), restated in numpy — one float32 operation per reference operation, in the
reference's order. Written from the reference, independently of kernels/faces.hip.h: vectorised over the queries with
boolean masks, the tables as the Python lists the caller authored (never the library's image).

Rust semantics kept: f32::clamp (`x < lo ? lo : x > hi ? hi : x`, so -0.0 stays -0.0), f32::max(0.0) before the cast to
usize, Vec3A::lerp as the project pins it through diffuse_color: a * (1 - s) + b * s."""
import numpy as np

f32, u32 = np.float32, np.uint32
NO_FACE = 0xFFFFFFFF
TRIANGLE, QUAD_LOWER, QUAD_UPPER, UNMAPPABLE = 0, 1, 2, 3


def _clamp01(x):
    x = np.asarray(x, f32)
    return np.where(x < f32(0), f32(0), np.where(x > f32(1), f32(1), x)).astype(f32)


def map_resolve(faces, slices, prim, u, v, swapped):
    """FaceMap::resolve over arrays: -> (face u32, fu, fv); `None` is (NO_FACE, 0, 0)."""
    faces, slices = np.asarray(faces, u32), np.asarray(slices, np.uint8)
    prim = np.asarray(prim, np.int64)
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    swapped = np.broadcast_to(np.asarray(swapped, bool), prim.shape)
    inside = prim < len(faces)
    at = np.where(inside, prim, 0)
    face = faces[at] if len(faces) else np.zeros(prim.shape, u32)
    sl = slices[at] if len(faces) else np.full(prim.shape, UNMAPPABLE, np.uint8)
    u, v = np.where(swapped, v, u), np.where(swapped, u, v)
    s = (u + v).astype(f32)
    fu = np.where(sl == QUAD_LOWER, s, u)
    fv = np.where(sl == QUAD_UPPER, s, v)
    some = inside & (sl != UNMAPPABLE)
    return (np.where(some, face, u32(NO_FACE)).astype(u32), np.where(some, _clamp01(fu), f32(0)).astype(f32),
            np.where(some, _clamp01(fv), f32(0)).astype(f32))


def world_resolve(maps, bindings, geom_id, prim, u, v):
    """World::intersect's lookup. maps: [(faces, slices)]; bindings: {geom_id: (map, swapped)}; a miss is geom_id ==
    0xFFFFFFFF. -> (face, fu, fv)."""
    geom_id = np.asarray(geom_id, np.int64)
    n = len(geom_id)
    face, fu, fv = np.full(n, NO_FACE, u32), np.zeros(n, f32), np.zeros(n, f32)
    for g, (m, swapped) in bindings.items():
        sel = np.nonzero(geom_id == g)[0]
        if len(sel):
            face[sel], fu[sel], fv[sel] = map_resolve(maps[m][0], maps[m][1], np.asarray(prim)[sel], np.asarray(u, f32)[sel],
                                                      np.asarray(v, f32)[sel], swapped)
    return face, fu, fv


def texture_eval(sizes, texels, fallback, face, u, v):
    """PtexColor::eval over arrays. sizes: [(width, height)] per face, the faces' texels packed in face order; texels
    float32 [n, 3]. -> float32 [len(face), 3]."""
    wh = np.asarray(sizes, np.int64).reshape(-1, 2)
    area = wh[:, 0] * wh[:, 1]
    offset = np.concatenate([[0], np.cumsum(area)[:-1]]).astype(np.int64) if len(wh) else np.zeros(0, np.int64)
    texels = np.asarray(texels, f32).reshape(-1, 3)
    face = np.asarray(face, np.int64)
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    out = np.empty((len(face), 3), f32)
    out[:] = np.asarray(fallback, f32)
    known = face < len(wh)
    at = np.where(known, face, 0)
    w = wh[at, 0] if len(wh) else np.zeros(len(face), np.int64)
    h = wh[at, 1] if len(wh) else np.zeros(len(face), np.int64)
    ok = known & (w > 0) & (h > 0)
    if not ok.any():
        return out
    w, h, off, u, v = w[ok], h[ok], offset[at[ok]], u[ok], v[ok]
    with np.errstate(invalid="ignore"):
        fu = np.where(np.isfinite(u), _clamp01(u), f32(0)).astype(f32)
        fv = np.where(np.isfinite(v), _clamp01(v), f32(0)).astype(f32)
    x = (fu * w.astype(f32) - f32(0.5)).astype(f32)
    y = (fv * h.astype(f32) - f32(0.5)).astype(f32)
    x0, y0 = np.floor(x).astype(f32), np.floor(y).astype(f32)
    tx, ty = (x - x0).astype(f32), (y - y0).astype(f32)

    def index(c, n):  # (c.max(0.0) as usize).min(n - 1)
        return np.minimum(np.maximum(c, f32(0)).astype(np.int64), n - 1)
    x0i, x1i = index(x0, w), index((x0 + f32(1)).astype(f32), w)
    y0i, y1i = index(y0, h), index((y0 + f32(1)).astype(f32), h)

    def texel(xi, yi):
        return texels[off + yi * w + xi]

    def lerp(a, b, s):
        s = s[:, None]
        return ((a * (f32(1) - s)).astype(f32) + (b * s).astype(f32)).astype(f32)
    top = lerp(texel(x0i, y0i), texel(x1i, y0i), tx)
    bot = lerp(texel(x0i, y1i), texel(x1i, y1i), tx)
    out[ok] = lerp(top, bot, ty)
    return out
