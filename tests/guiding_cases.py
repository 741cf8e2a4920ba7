"""Named guiding fields and queries for tests/test_guiding.py (CPU) and tests/test_gpu_guiding.py: the configuration and
the training passes of every case as seeded numpy arrays, the random and the hand-made query lists, and the guided
bounce's truth — sample_bounce_direction (tracer.rs:777-826) composed from the restatement (tests/guiding_ref.py), the
oracle's drivers (tests/ora.py: ora_t_new_domain, ora_t_draw4, ora_t_scatter_n, ora_t_eval_n, ora_interior_medium) and a
few lines restating make_ray (openpbr.rs:1186-1200, material.rs:79-81).

Bounds are [-5, 5]^3, where seam_cases.shade_queries puts its points. Everything is derived from
numpy.random.default_rng with fixed seeds; nothing here reads the library."""
import ctypes as C

import numpy as np

import guiding_ref as gr
import seam_cases as sc

f32, u32 = np.float32, np.uint32
BMIN, BMAX = np.full(3, -5.0, f32), np.full(3, 5.0, f32)
CASES = ("untrained", "one_leaf", "octant", "sharp_cone", "deep_spatial", "one_point", "zero_flux", "edges")


def unit(rng, n):
    v = rng.normal(size=(n, 3)).astype(f32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def uniform_sphere(rng, n):
    z = rng.uniform(-1, 1, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(f32)


def make_samples(pos, direction, radiance=1.0):
    out = np.zeros(len(pos), gr.SAMPLE)
    out["pos"], out["dir"] = np.asarray(pos, f32), np.asarray(direction, f32)
    out["radiance"] = radiance
    return out


def _positions(rng, n):
    return rng.uniform(-5, 5, size=(n, 3)).astype(f32)


def octant_pass(rng, n):  # dtree.rs:331-344: all flux inside one octant of the sphere
    d = np.abs(uniform_sphere(rng, n))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def cone_pass(rng, n):  # dtree.rs:401-410: a tight cone around +z plus a dim uniform background
    v = rng.uniform(size=(n, 2))
    cone = np.stack([0.05 * (v[:, 0] - 0.5), 0.05 * (v[:, 1] - 0.5), np.ones(n)], axis=1)
    cone /= np.linalg.norm(cone, axis=1, keepdims=True)
    return np.where((rng.uniform(size=n) < 0.9)[:, None], cone, uniform_sphere(rng, n)).astype(f32)


def case(name):
    """(config overrides, [(SAMPLE records, next_iteration), ...]) of a named field."""
    rng = np.random.default_rng(7000 + CASES.index(name))
    if name == "untrained":  # a field that has received no samples: one empty pass
        return {}, [(np.zeros(0, gr.SAMPLE), 1)]
    if name == "one_leaf":
        d = unit(rng, 1000) * f32(0.2) + np.array([0, 0, 1], f32)
        return dict(spatial_c=4000.0), [(make_samples(_positions(rng, 1000), d), 1)]
    if name == "octant":
        return {}, [(make_samples(_positions(rng, 20000), octant_pass(rng, 20000)), k + 1) for k in range(4)]
    if name == "sharp_cone":
        return {}, [(make_samples(_positions(rng, 5000), cone_pass(rng, 5000)), k + 1) for k in range(8)]
    if name == "deep_spatial":
        centres = np.array([[2.5, -1.0, 3.0], [-4.0, -4.0, 0.5]], f32)
        passes = []
        for k in range(5):
            pos = (centres[rng.integers(0, 2, 600)] + rng.normal(scale=0.25, size=(600, 3))).astype(f32)
            passes.append((make_samples(pos, octant_pass(rng, 600), rng.uniform(0.1, 3.0, 600).astype(f32)), k + 1))
        return dict(spatial_c=4.0), passes
    if name == "one_point":
        pos = np.tile(np.array([[1.25, -2.5, 3.75]], f32), (2000, 1))
        d = np.tile(np.array([[0.3, -0.5, 0.8]], f32), (2000, 1))
        return dict(spatial_c=4.0, spatial_max_depth=5, dtree_max_depth=8), [(make_samples(pos, d), k + 1) for k in range(4)]
    if name == "zero_flux":  # counted (the spatial tree splits), never splat
        rad = np.array([0.0, np.nan, -1.0], f32)[rng.integers(0, 3, 900)]
        return dict(spatial_c=16.0), [(make_samples(_positions(rng, 900), unit(rng, 900), rad), k + 1) for k in range(2)]
    if name == "edges":  # on the hull, on the padded hull, outside both, exactly on split planes
        pad = f32(10.0) * f32(1e-3)
        lo, hi = f32(-5.0) - pad, f32(5.0) + pad
        marks = np.array([-7.0, lo, -5.0, -2.5, 0.0, 2.5, 5.0, hi, 7.0], f32)  # 0 and +-2.5: midpoints of the padded box
        marks[3], marks[5] = f32(0.5) * (lo + f32(0.0)), f32(0.5) * (f32(0.0) + hi)
        grid = np.stack(np.meshgrid(marks, marks, marks, indexing="ij"), axis=-1).reshape(-1, 3)
        passes = []
        for k in range(3):
            pos = np.concatenate([grid, _positions(rng, 300)]).astype(f32)
            passes.append((make_samples(pos, unit(rng, len(pos)), rng.uniform(0.0, 2.0, len(pos)).astype(f32)), k + 1))
        return dict(spatial_c=20.0), passes
    raise KeyError(name)


def build_ref(name, h, upto=None):
    """The restatement's field after `upto` passes (all of them by default), and the list of its states' stats."""
    cfg, passes = case(name)
    field = gr.Field(BMIN, BMAX, cfg, h)
    for samples, it in passes[:upto]:
        field.update(samples, it)
    return field


def random_queries(n, rng):
    q = np.zeros(n, gr.QUERY)
    q["pos"] = rng.uniform(-6, 6, size=(n, 3)).astype(f32)
    q["dir"] = unit(rng, n) * rng.uniform(0.5, 2.0, size=(n, 1)).astype(f32)
    q["seed_u"], q["seed_v"] = rng.uniform(size=n).astype(f32), rng.uniform(size=n).astype(f32)
    return q


def edge_queries(split_planes=()):
    """The hand-made list: positions at and beyond the bounds, on split planes, +-inf and NaN; directions +-axes, zero,
    NaN and unnormalised; seeds 0, 1 - 2^-24, 0.5 and NaN."""
    pad = f32(10.0) * f32(1e-3)
    inf, nan = f32(np.inf), f32(np.nan)
    pos = [[-5, -5, -5], [5, 5, 5], [f32(-5) - pad] * 3, [f32(5) + pad] * 3, [-7, 0, 9], [100, -100, 100], [0, 0, 0], [0, 1, -1],
           [inf, 0, 0], [-inf, inf, 1], [nan, 0, 0], [nan, nan, nan], [1, nan, -inf]]
    for s in list(split_planes)[:8]:
        pos += [[s, s, s], [np.nextafter(f32(s), -inf), s, np.nextafter(f32(s), inf)]]
    dirs = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [nan, 0, 1], [nan, nan, nan], [3, -4, 12],
            [1e-30, 0, 0], [-1, -0.0, 0], [-1, 0.0, 0], [inf, 1, 0]]
    seeds = [f32(0.0), f32(1.0) - f32(2.0 ** -24), f32(0.5), nan]
    rows = [(p, d, su, sv) for p in pos for d in dirs for su in seeds for sv in seeds]
    q = np.zeros(len(rows), gr.QUERY)
    q["pos"] = np.array([r[0] for r in rows], f32)
    q["dir"] = np.array([r[1] for r in rows], f32)
    q["seed_u"] = np.array([r[2] for r in rows], f32)
    q["seed_v"] = np.array([r[3] for r in rows], f32)
    return q


def queries(field, n, seed):
    """n random queries followed by the hand-made list with the field's own split planes."""
    fl = field.flat()
    planes = np.unique(fl.split[fl.axis != gr.NO_CHILD])
    return np.concatenate([random_queries(n, np.random.default_rng(seed)), edge_queries(planes)])


# ---- the guided bounce's truth ------------------------------------------------------------------------------------------
EXITS = ("untrained", "guide", "guide_fallback", "bsdf_delta", "bsdf_continuous")


def _oracle():
    import ora
    return ora, ora.lib()


def has_interior(mats):
    """interior_medium().is_some() per material (openpbr.rs:225-259), from the oracle."""
    ora, L = _oracle()
    out = np.zeros(len(mats), bool)
    med = ora.Medium()
    for i, m in enumerate(mats):
        rec = ora.Material.from_buffer_copy(m.tobytes())
        out[i] = m["kind"] == 0 and L.ora_interior_medium(C.byref(rec), C.byref(med)) != 0
    return out


def domains(q):
    """new_domain(v, K_BSDF = 2), new_domain(v, K_GUIDE = 3) and draw_sample_f32::<4> of the latter, from the oracle."""
    _, L = _oracle()
    pat, idx = q["sampler_pattern"], q["sampler_index"]
    bsdf = np.array([L.ora_t_new_domain(int(p), 2) for p in pat], u32)
    guide = np.array([L.ora_t_new_domain(int(p), 3) for p in pat], u32)
    gs = np.zeros((len(q), 4), f32)
    buf = (C.c_float * 4)()
    for i in range(len(q)):
        L.ora_t_draw4(int(guide[i]), int(idx[i]), buf)
        gs[i] = buf[:]
    return bsdf, gs


def make_ray(mats, q, wi, interior):
    """Material::make_ray: (origin, medium flag)."""
    m = mats[q["material"]]
    n = q["normal"]
    with np.errstate(all="ignore"):
        ndw = (n[:, 0] * wi[:, 0] + n[:, 1] * wi[:, 1]) + n[:, 2] * wi[:, 2]
        across = (m["kind"] == 0) & (m["transmission_weight"] > 0) & (m["thin_walled"] == 0) & (ndw < 0)
        origin = np.where(across[:, None], q["p"] + wi * f32(1e-4), q["p"]).astype(f32)
    medium = across & (q["front_face"] != 0) & interior[q["material"]]
    return origin, medium


def guided_truth(field, mats, q):
    """sample_bounce_direction for every query -> (SCATTER_SAMPLE records as crt_material_scatter_guided_n writes them,
    the exit each call took as an index into EXITS)."""
    drv = sc.oracle_drivers()
    fl = field.flat()
    alpha = fl.alpha
    bsdf_pat, gs = domains(q)
    qb = q.copy()
    qb["sampler_pattern"] = bsdf_pat
    plain = drv.scatter(mats, qb)
    root = fl.dtree_at(q["p"])
    trained = gr.DTree.total(fl.sums[root]) > 0
    out = plain.copy()
    exits = np.zeros(len(q), np.int64)
    coin = trained & (gs[:, 0] < alpha)
    # guide branch
    some_g, p0, p1, p_guide = fl.dtree_sample(root, np.ascontiguousarray(gs[:, 1]), np.ascontiguousarray(gs[:, 2]))
    wi = field.maps.canonical_to_dir(p0, p1)
    qe = q.copy()
    qe["wi"] = np.where(some_g[:, None], wi, q["wi"])
    ev = drv.eval(mats, qe)
    guide = coin & some_g & (ev["some"] == 1)
    origin, medium = make_ray(mats, q, wi, has_interior(mats))
    with np.errstate(all="ignore"):
        pdf = gr.rmax(alpha * p_guide + (f32(1.0) - alpha) * ev["pdf"], f32(1e-4))
    out["origin"][guide] = origin[guide]; out["dir"][guide] = wi[guide]; out["value"][guide] = ev["value"][guide]
    out["pdf"][guide] = pdf[guide]; out["some"][guide] = 1
    out["flags"][guide] = np.where(medium, 2, 0)[guide]
    exits[coin & ~guide] = 2
    exits[guide] = 1
    # BSDF branch
    b = trained & ~coin & (plain["some"] == 1)
    delta = b & ((plain["flags"] & 1) != 0)
    with np.errstate(all="ignore"):
        out["value"][delta] = (plain["value"] / (f32(1.0) - alpha)).astype(f32)[delta]
        d = plain["dir"]
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        wn = (d / length[:, None]).astype(f32)
    qc = q.copy()
    qc["wi"] = np.where(b[:, None] & ~delta[:, None], wn, q["wi"])
    evc = drv.eval(mats, qc)
    cont = b & ~delta & (evc["some"] == 1)
    c0, c1 = field.maps.dir_to_canonical(wn)
    with np.errstate(all="ignore"):
        pg = fl.dtree_pdf(root, c0, c1)
        mix = gr.rmax(alpha * pg + (f32(1.0) - alpha) * plain["pdf"], f32(1e-4))
    out["pdf"][cont] = mix[cont]
    exits[trained & ~coin] = 4
    exits[delta] = 3
    out["flags"] = out["flags"] | np.where(trained, 4, 0).astype(u32) | np.where(guide, 8, 0).astype(u32)
    return out, exits
