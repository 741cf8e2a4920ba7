"""Seeded cases for the volume aggregate, shared by tests/test_volumes.py (host twin against the restatement) and
tests/test_gpu_volumes.py (kernels against the restatement): the smallest shapes at which this code can go wrong.

Aggregates: a unit cube at identity; a cube scaled x2 in x and translated; a cube rotated 45 degrees about z; two
overlapping homogeneous boxes; homogeneous + grid overlapping (ratio tracking across a homogeneous span); eight regions
nested around one point (the lobe array full); a region with zero coefficients (skipped). Grids 1x1x1, 2x2x2 (0..7),
3x5x2 (distinct values: index order), smoke.usda's 4x4x4. Noise with smoke.usda's parameters and with one octave at
threshold 0.999. Chromatic coefficients, sigma_s = 0, sigma_a = 0 and grey, emission on and off.
Segments: origin outside, inside and on a face; missing the box; parallel to each axis inside and outside the slab;
t_max before the box, inside it, behind it and inf; t_eps > t_max.
Density points: exactly on +-half, one ulp outside, u within half a voxel of each edge, NaN, +-1e30."""
import numpy as np

f32, u32 = np.float32, np.uint32

SMOKE_GRID = [0.000, 0.092, 0.092, 0.000, 0.092, 0.309, 0.309, 0.092, 0.092, 0.309, 0.309, 0.092, 0.000, 0.092, 0.092, 0.000,
              0.092, 0.309, 0.309, 0.092, 0.309, 0.639, 0.639, 0.309, 0.309, 0.639, 0.639, 0.309, 0.092, 0.309, 0.309, 0.092,
              0.092, 0.309, 0.309, 0.092, 0.309, 0.639, 0.639, 0.309, 0.309, 0.639, 0.639, 0.309, 0.092, 0.309, 0.309, 0.092,
              0.000, 0.092, 0.092, 0.000, 0.092, 0.309, 0.309, 0.092, 0.092, 0.309, 0.309, 0.092, 0.000, 0.092, 0.092, 0.000]
GRID_352 = [round(0.05 + 0.031 * k, 3) for k in range(30)]  # 3 x 5 x 2, every value distinct


def affine(scale=(1, 1, 1), rot_z_deg=0.0, translate=(0, 0, 0)):
    """translate * rotate_z * scale as 12 floats: three columns, then the translation."""
    c, s = np.cos(np.radians(rot_z_deg)), np.sin(np.radians(rot_z_deg))
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    m = rot @ np.diag(scale)
    return np.concatenate([m[:, 0], m[:, 1], m[:, 2], translate]).astype(f32)


def aggregates(V):
    """name -> list of region dicts (V = the package's volumes module)."""
    R = V.region
    smoke = dict(field="noise", noise_scale=4, noise_octaves=4, noise_gain=0.5, noise_lacunarity=2, noise_threshold=0.25, noise_seed=42)
    out = {
        "unit_chromatic": [R(sigma_s=(0.7, 0.5, 0.9), sigma_a=(0.2, 0.4, 0.9), g=0.3, emission=(4.0, 1.5, 0.3))],
        "scaled_grey": [R(local_to_world=affine((2, 1, 1), 0, (5, 0, 0)), half_extent=1.0, sigma_s=1.0, sigma_a=0.0)],
        "rotated_noise": [R(local_to_world=affine((1, 1, 1), 45, (0, 0, 0)), half_extent=1.0, sigma_s=(2.0, 1.5, 1.0), sigma_a=0.3, g=-0.4, **smoke)],
        "overlap_homogeneous": [R(sigma_s=0.0, sigma_a=0.5), R(local_to_world=affine(translate=(0.25, 0, 0)), sigma_s=0.0, sigma_a=0.75)],
        "homogeneous_and_grid": [R(half_extent=(1.0, 0.5, 0.5), sigma_s=0.4, sigma_a=0.1, g=0.5),
                                 R(local_to_world=affine(translate=(0.4, 0.1, 0)), sigma_s=(0.3, 0.2, 0.1), sigma_a=0.05, g=-0.2,
                                   field="grid", grid_dims=(2, 2, 2), grid_data=list(range(8)))],
        "sigma_s_zero": [R(sigma_s=0.0, sigma_a=(0.8, 0.5, 0.2), emission=(1.0, 2.0, 3.0), field="grid", grid_dims=(1, 1, 1), grid_data=[0.6])],
        "zero_coefficients": [R(sigma_s=0.0, sigma_a=0.0), R(local_to_world=affine(translate=(0.1, 0, 0)), sigma_s=1.3, sigma_a=0.0,
                                                                 field="grid", grid_dims=(3, 5, 2), grid_data=GRID_352)],
        "noise_one_octave": [R(sigma_s=3.0, sigma_a=0.5, density_scale=40.0, field="noise", noise_scale=3.0, noise_octaves=1, noise_gain=0.5,
                               noise_lacunarity=2.0, noise_threshold=0.999, noise_seed=7)],
        "smoke": [R(local_to_world=affine((0.9, 1.6, 0.9), 0, (-0.4, 1.7, 0)), half_extent=1.0, sigma_s=0.8, sigma_a=0.08, g=0.2, density_scale=12, **smoke),
                  R(local_to_world=affine(translate=(0.9, 0.3, 0.4)), half_extent=0.25, sigma_s=0.05, sigma_a=(0.6, 0.35, 0.15),
                    emission=(6, 2.2, 0.5), density_scale=4),
                  R(local_to_world=affine(translate=(1.1, 2.6, -0.8)), half_extent=0.5, sigma_s=0.7, sigma_a=0.05, density_scale=6,
                    field="grid", grid_dims=(4, 4, 4), grid_data=SMOKE_GRID)],
    }
    nested = []
    for k in range(8):  # eight boxes around the origin, every field kind, every one scattering: the lobe array is full
        kw = dict(local_to_world=affine((1 + 0.1 * k, 1, 1), 11.0 * k, (0.02 * k, -0.01 * k, 0)), half_extent=0.4 + 0.1 * k,
                  sigma_s=(0.3 + 0.05 * k, 0.2, 0.25), sigma_a=0.02 * k, g=-0.7 + 0.2 * k, emission=(0.1 * k, 0.0, 0.2))
        if k % 3 == 1:
            kw.update(smoke, noise_seed=k)
        if k % 3 == 2:
            kw.update(field="grid", grid_dims=(3, 5, 2) if k == 2 else ((1, 1, 1) if k == 5 else (4, 4, 4)),
                      grid_data=GRID_352 if k == 2 else ([0.8] if k == 5 else SMOKE_GRID))
        nested.append(R(**kw))
    out["nested_eight"] = nested
    return out


def segments(V, n, seed, centre=(0, 0, 0), extent=2.5):
    """n QUERY records: the hand-made segments first (as many as fit), then seeded random ones around `centre`."""
    rng = np.random.default_rng(seed)
    q = np.zeros(n, V.QUERY)
    c = np.asarray(centre, f32)
    o = (c + rng.uniform(-extent, extent, (n, 3))).astype(f32)
    inside = rng.random(n) < 0.3
    o[inside] = (c + rng.uniform(-0.45, 0.45, (int(inside.sum()), 3))).astype(f32)
    target = c + rng.uniform(-0.6, 0.6, (n, 3))
    d = target - o
    miss = rng.random(n) < 0.15
    d[miss] = rng.normal(size=(int(miss.sum()), 3))
    length = np.linalg.norm(d, axis=1, keepdims=True)
    d = d / np.where(length > 0, length, 1)
    d *= np.where(rng.random((n, 1)) < 0.25, rng.uniform(0.3, 3.0, (n, 1)), 1.0)  # the direction is not always unit
    axis = rng.random(n) < 0.2  # parallel to an axis: the 1e-9 skip, inside the slab and outside it
    ax = rng.integers(0, 3, n)
    d[axis] = 0
    d[axis, ax[axis]] = np.where(rng.random(int(axis.sum())) < 0.5, 1.0, -1.0)
    t_max = rng.choice(np.array([0.5, 1.5, 2.5, 10.0, np.inf]), n)
    t_eps = np.where(rng.random(n) < 0.05, 20.0, 1e-3)  # t_eps > t_max
    q["origin"], q["direction"], q["t_eps"], q["t_max"] = o, d.astype(f32), t_eps, t_max
    q["seed"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(u32)
    hand = [  # origin, direction, t_eps, t_max (relative to centre)
        ((-2, 0, 0), (1, 0, 0), 1e-3, 10.0), ((-2, 0, 0), (1, 0, 0), 1e-3, 1.0), ((-2, 0, 0), (1, 0, 0), 1e-3, 2.0),
        ((-2, 0, 0), (1, 0, 0), 1e-3, np.inf), ((0, 0, 0), (1, 0, 0), 1e-3, np.inf), ((0.5, 0, 0), (1, 0, 0), 1e-3, 10.0),
        ((0.5, 0, 0), (-1, 0, 0), 1e-3, 10.0), ((-2, 0.5, 0), (1, 0, 0), 1e-3, 10.0), ((-2, 0.75, 0), (1, 0, 0), 1e-3, 10.0),
        ((0, -2, 0.2), (0, 1, 0), 1e-3, 10.0), ((0.1, 0.2, -2), (0, 0, 1), 1e-3, 10.0), ((0, 0, -2), (0, 0, -1), 1e-3, 10.0),
        ((-2, 0, 0), (1, 0, 0), 5.0, 1.0), ((-2, 0, 0), (2, 0, 0), 1e-3, 10.0), ((-2, -2, -2), (1, 1, 1), 1e-3, 10.0),
        ((-2, 0, 0), (1, 1e-10, 0), 1e-3, 10.0), ((0, 0, 0), (0, 1e-10, 1), 1e-3, 3.0),
    ]
    for k, (oo, dd, te, tm) in enumerate(hand[:n]):
        q["origin"][k], q["direction"][k], q["t_eps"][k], q["t_max"][k] = c + np.asarray(oo, f32), dd, te, tm
    return q


def phase_numbers(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(f32)


def density_points(rec, n, seed):
    """World points for VolumeRegion::density of one REGION record whose placement is a translation (or identity): on
    +-half, one ulp outside, within half a voxel of each edge, NaN, +-1e30, then seeded random ones."""
    rng = np.random.default_rng(seed)
    h = np.asarray(rec["half_extent"], f32)
    t = np.asarray(rec["local_to_world"], f32)[9:12]
    pts = []
    for a in range(3):
        for sgn in (-1.0, 1.0):
            p = np.zeros(3, f32)
            p[a] = f32(sgn) * h[a]
            pts.append(p.copy())
            p[a] = np.nextafter(p[a], f32(sgn * np.inf), dtype=f32)
            pts.append(p.copy())
            for frac in (0.01, 0.12, 0.24):  # inside the first / last half voxel of a 2- or 4-cell axis
                p = (rng.uniform(-1, 1, 3) * h).astype(f32)
                p[a] = f32(sgn) * h[a] * f32(1.0 - 2.0 * frac)
                pts.append(p)
    pts = [p + t for p in pts]
    pts += [np.array([np.nan, 0, 0], f32), np.array([0, np.nan, np.nan], f32), np.array([1e30, 0, 0], f32), np.array([0, -1e30, 1e30], f32),
            np.array([np.inf, 0, 0], f32), t.copy()]
    rnd = (t + rng.uniform(-1.2, 1.2, (max(n - len(pts), 0), 3)) * h).astype(f32)
    return np.concatenate([np.asarray(pts, f32), rnd])[:max(n, len(pts))]


def step_limit_aggregate(V):
    """A pure-null-collision walk that ends by itself: a unit cube whose 1x1x4 grid is zero below u.z = 0.375 and 1 at
    its top voxel, so the majorant is sigma while the density along a segment at u.z = 0.2 is exactly 0. With
    sigma = 4 * MAX_STEPS the majorant optical depth over the unit segment is 4 * MAX_STEPS: the reference's walk would
    take about that many candidates and finish; the bounded walk stops at MAX_STEPS with the step-limit status."""
    sigma = 4.0 * V.MAX_STEPS
    regions = [V.region(sigma_s=sigma, sigma_a=0.0, field="grid", grid_dims=(1, 1, 4), grid_data=[0.0, 0.0, 0.0, 1.0])]
    q = np.zeros(1, V.QUERY)
    q["origin"], q["direction"], q["t_eps"], q["t_max"], q["seed"] = (-2.0, 0.0, -0.3), (1.0, 0.0, 0.0), 1e-3, 10.0, 12345
    return regions, q
