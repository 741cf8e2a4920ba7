"""Maps and queries for the environment-map tests (test infrastructure; tests/env_ref.py holds the truth).

MAPS: name -> (width, height, rgb [h, w, 3] float32, light_to_world 3x3 or None). Chosen for the paths the code can
take: a single texel, a size that is no power of two, zero texels / a whole zero row / adjacent zero bins (duplicate CDF
entries and the uniform-row fallback), a black map (sample declines), the reference's own spotty maps, uniform maps,
the sample scene's HDRI under identity and under the scene's rotateY 20, and a non-orthogonal light_to_world."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_F = lambda a: np.ascontiguousarray(a, dtype=f32)


def spotty(w, h, bx, by):
    """environment.rs:223-227"""
    px = np.full((h, w, 3), 0.05, dtype=f32)
    px[by, bx] = 500.0
    return px


def rotate_y(deg):
    """The matrix whose columns are the images of the axes under USD's rotateY (usda.py builds the same from the prim)."""
    a = np.deg2rad(deg)
    c, s = f32(np.cos(a)), f32(np.sin(a))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=f32)


def hand_8x4():
    rng = np.random.default_rng(7)
    px = rng.uniform(0.1, 2.0, size=(4, 8, 3)).astype(f32)
    px[0, 2] = 0.0                 # a zero texel
    px[1, 3] = px[1, 4] = 0.0      # two adjacent zero bins: cdf[3] == cdf[4] == cdf[5]
    px[1, 0] = 0.0                 # a zero first bin: cdf[0] == cdf[1] == 0
    px[1, 7] = 0.0                 # a zero last bin: cdf[7] == cdf[8] == 1
    px[2] = 0.0                    # a whole zero row: uniform conditional CDF, conditional pdf 1, marginal weight 0
    px[3, 5] = (-1.0, -2.0, -0.5)  # a negative texel: weight 0, radiance as authored
    return px


def sky_env(crt):
    return np.ascontiguousarray(crt.exr.read_exr(os.path.join(ROOT, "scenes", "sky_env.exr")), dtype=f32)


def maps(crt):
    """crt: the package (its EXR reader decodes scenes/sky_env.exr)."""
    sky = sky_env(crt)
    return {
        "1x1": (1, 1, np.full((1, 1, 3), 0.7, f32), None),
        "3x2": (3, 2, np.random.default_rng(3).uniform(0.0, 4.0, size=(2, 3, 3)).astype(f32), None),
        "hand_8x4": (8, 4, hand_8x4(), None),
        "black_8x4": (8, 4, np.zeros((4, 8, 3), f32), None),
        "spotty_64x32": (64, 32, spotty(64, 32, 40, 8), None),
        "spotty_32x16": (32, 16, spotty(32, 16, 20, 6), None),
        "uniform_32x16": (32, 16, np.ones((16, 32, 3), f32), None),
        "uniform_64x32": (64, 32, np.ones((32, 64, 3), f32), None),
        "sky_env": (sky.shape[1], sky.shape[0], sky, None),
        "sky_env_rotY20": (sky.shape[1], sky.shape[0], sky, rotate_y(20.0)),
        "skewed_3x2": (3, 2, np.random.default_rng(5).uniform(0.0, 4.0, size=(2, 3, 3)).astype(f32),
                       np.array([[1.0, 0.3, 0.0], [0.1, 0.9, -0.2], [0.0, 0.25, 1.2]], dtype=f32)),
    }


TINT = np.array([1.25, 0.5, 2.0], dtype=f32)


def edge_directions(ref):
    """+-X +-Y +-Z, the u seam (d.x = +-0 with d.z > 0), directions through texel corners, NaN components."""
    d = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
         (0.0, 0.0, 1.0), (-0.0, 0.0, 1.0), (0.0, 0.5, 0.8660254), (-0.0, -0.5, 0.8660254),
         (np.nan, 0, 1), (0, np.nan, 1), (1, 0, np.nan), (np.nan, np.nan, np.nan)]
    d = np.array(d, dtype=f32)
    xs, ys = np.meshgrid(np.arange(ref.w + 1, dtype=f32) / f32(ref.w), np.arange(ref.h + 1, dtype=f32) / f32(ref.h))
    corners = ref.uv_to_direction(xs.reshape(-1), ys.reshape(-1))
    return np.concatenate([d, corners]).astype(f32)


def edge_uv(ref):
    """(u, v) pairs at the edges of the inversion: u and v equal to 0, to 1 - 2^-24 and to CDF entries exactly (the
    duplicated ones of zero-weight bins included), each with its two float32 neighbours. Every row's conditional entries
    are paired with a v that selects that row, every marginal entry with a few u; then NaN, 1.0 and negative numbers."""
    one_m = f32(1.0) - f32(2.0 ** -24)

    def around(c):
        c = np.unique(np.concatenate([[f32(0), one_m], _F(c)]).astype(f32))
        c = np.unique(np.concatenate([c, np.nextafter(c, f32(-1)), np.nextafter(c, f32(2))]).astype(f32))
        return c[(c >= 0) & (c < 1)]

    us, vs = [], []
    for y in range(ref.h):
        c0, c1 = ref.marg_cdf[y], ref.marg_cdf[y + 1]
        if not c1 > c0:
            continue  # a row of weight 0 is never selected
        u = around(ref.cond_cdf[y])
        for v in (c0, f32(f32(0.5) * c0 + f32(0.5) * c1)):
            us.append(u)
            vs.append(np.full(len(u), v, f32))
    v = around(ref.marg_cdf)
    for u in (f32(0), f32(0.5), one_m):
        us.append(np.full(len(v), u, f32))
        vs.append(v)
    extra = np.array([[np.nan, 0.5], [0.5, np.nan], [np.nan, np.nan], [1.0, 1.0], [-0.25, 0.5], [0.5, -0.25]], dtype=f32)
    us.append(extra[:, 0])
    vs.append(extra[:, 1])
    return np.concatenate(us).astype(f32), np.concatenate(vs).astype(f32)


def random_directions(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
