"""Do the sampling routines draw from the density they report? Shared by tests/test_scatter_density.py (the oracle and
the host-compiled device source) and tests/test_gpu_scatter_density.py (the device): any seam_cases.Drivers-shaped object
goes in, the statistics come out.

For one material and one view direction, N = 65 536 scatter draws with distinct (sampler_pattern, sampler_index) (indices
0..255 under 256 patterns, as a renderer walks them) are
  * binned on a 16 x 32 grid in (cos theta, phi) over both hemispheres and compared, by Pearson's chi-square, with
    N * integral over the cell of the pdf that eval reports (8 x 8 Gauss points per cell, float64);
  * averaged as value * cos / pdf (the tracer's bounce factor, tracer.rs:1461-1471) and compared with the float64
    quadrature of eval's value * cos over a 256 x 512 grid: integral f cos^2 domega.

The reported pdf is the density of the draw that RETURNS a sample (a VNDF draw whose reflection dips below the surface
returns none, openpbr.rs:1026-1136), so it integrates to the returned fraction, not to one: the expected count of a cell
is N times its integral with no further factor, and that the integral over the sphere equals the returned fraction is
checked on its own.

The floor pdf.max(1e-4) (openpbr.rs:1128, :1155) is part of the reported value and no density: where eval reports the
floor, the expected density is pdf_all unfloored (the oracle's ora_pdf_all: the three sides of the comparison agree bit
for bit, tests/test_shading_seam_host.py and tests/test_gpu_shading_seam.py), and the draws that report the floor are
counted.

The hit frame: normal +z at the origin, the viewer in the x-z plane; openpbr.rs:268-285 builds tangent (1,0,0) and
bitangent (0,1,0) over that normal, so world coordinates are the local ones."""
import ctypes as C

import numpy as np
from scipy import stats

import seam_cases as sc

N = 65536
BLOCKS = 16
VIEWS = (1.0, 0.7, 0.3, 0.1)
N_MU, N_PHI, GAUSS = 16, 32, 8
MIN_EXPECTED = 20.0
P_MIN = 1e-4
MAX_LEFT_OUT = 0.01
FLOOR = np.float32(1e-4)


def material(**over):
    """OpenPBR::default (openpbr.rs:130-173) with the given inputs."""
    import ora
    m = np.frombuffer(bytes(ora.default_material()), dtype=sc.MATERIAL).copy()
    for k, v in over.items():
        m[k] = v
    return m


def lambert(roughness, ior):
    """The slab of tests/radiometry_cases.py: the configuration that shows the furnace gain."""
    return material(base_color=0.5, base_weight=1.0, specular_weight=0.0, base_diffuse_roughness=0.0,
                    specular_roughness=roughness, specular_ior=ior)


# One hand-picked material per lobe class. Roughness 0.35 and up: the lobes must be wide enough for 8 x 8 Gauss points in
# a cell of 0.125 x 0.196 and for the 256 x 512 grid to integrate them (alpha = 0.12: a lobe some 20 grid cells across).
MATERIALS = {
    "base": dict(base_color=(0.7, 0.5, 0.3), specular_roughness=0.4, base_diffuse_roughness=0.3),
    "metal": dict(base_metalness=1.0, base_color=(0.9, 0.6, 0.3), specular_roughness=0.7),
    "anisotropic": dict(base_metalness=0.6, specular_roughness=0.5, specular_roughness_anisotropy=0.6),
    "coat": dict(coat_weight=0.8, coat_roughness=0.35, specular_roughness=0.5, base_color=(0.6, 0.2, 0.2)),
    "fuzz": dict(fuzz_weight=0.7, fuzz_roughness=0.5, specular_roughness=0.5, fuzz_color=(0.8, 0.8, 0.9)),
    "transmission": dict(transmission_weight=0.6, specular_roughness=0.7, transmission_color=(0.9, 0.95, 1.0)),
}
LAMBERTS = {"lambert_r%g_ior%g" % (r, i): (r, i) for r in (0.05, 0.3, 1.0) for i in (1.0, 1.5)}


def named(name):
    return lambert(*LAMBERTS[name]) if name in LAMBERTS else material(**MATERIALS[name])


def queries(cos_v, n):
    q = np.zeros(n, dtype=sc.SHADE_QUERY)
    q["ray_dir"] = (-np.sqrt(1.0 - cos_v * cos_v), 0.0, -cos_v)
    q["normal"] = (0.0, 0.0, 1.0)
    q["front_face"] = 1
    q["t"] = 1.0
    return q


def draws(drv, mat, cos_v):
    q = queries(cos_v, N)
    k = np.arange(N, dtype=np.uint64)
    q["sampler_pattern"] = (((k >> 8) + 1) * 2654435761 % (1 << 32)).astype(np.uint32)  # 256 patterns, Knuth's multiplier
    q["sampler_index"] = (k & 255).astype(np.uint32)
    return drv.scatter(mat, q)


def _unfloored(mat, cos_v, dirs):
    import ora
    m = ora.Material.from_buffer_copy(mat.tobytes())
    v = ora.V3(float(np.sqrt(1.0 - cos_v * cos_v)), 0.0, float(cos_v))
    f = ora.lib().ora_pdf_all
    return np.array([f(C.byref(m), v, ora.V3(float(d[0]), float(d[1]), float(d[2])), 1) for d in dirs], np.float64)


def reported(drv, mat, cos_v, dirs):
    """eval at the unit directions dirs [n, 3] -> (pdf as a density: unfloored where the floor is reported, value * |cos|
    as eval returns it [n, 3], how many directions reported the floor)."""
    q = queries(cos_v, len(dirs))
    q["wi"] = dirs.astype(np.float32)
    e = drv.eval(mat, q)
    assert e["some"].all()
    pdf = e["pdf"].astype(np.float64)
    hit = e["pdf"] == FLOOR
    if hit.any():
        pdf[hit] = _unfloored(mat, cos_v, q["wi"][hit])
        assert (pdf[hit] <= float(FLOOR) * (1 + 1e-6)).all()
    return pdf, e["value"].astype(np.float64), int(hit.sum())


def _grid(n_mu, n_phi, n_gauss):
    """Tensor Gauss-Legendre rule over [-1, 1] x [0, 2 pi) in n_mu x n_phi cells, n_gauss x n_gauss nodes a cell ->
    (unit directions [cells, nodes, 3], weights [cells, nodes]). In the two polar rows mu runs as +-(1 - dmu s^2): a lobe
    about the normal (a view along it, or its refraction) is a smooth function of theta ~ sqrt(2 dmu) s, not of mu."""
    x, w = np.polynomial.legendre.leggauss(n_gauss)
    x, w = (x + 1) / 2, w / 2                                            # on [0, 1]
    dmu, dphi = 2.0 / n_mu, 2.0 * np.pi / n_phi
    mu = -1.0 + dmu * (np.arange(n_mu)[:, None] + x[None, :])            # [n_mu, g]
    wmu = np.tile(w * dmu, (n_mu, 1))
    mu[0], wmu[0] = -1.0 + dmu * x * x, 2.0 * x * w * dmu
    mu[-1], wmu[-1] = 1.0 - dmu * x * x, 2.0 * x * w * dmu
    phi = dphi * (np.arange(n_phi)[:, None] + x[None, :])                # [n_phi, g]
    M = mu[:, None, :, None]
    P = phi[None, :, None, :]
    sn = np.sqrt(np.maximum(1.0 - M * M, 0.0))
    d = np.stack(np.broadcast_arrays(sn * np.cos(P), sn * np.sin(P), M), axis=-1)   # [n_mu, n_phi, g, g, 3]
    wt = wmu[:, None, :, None] * (w * dphi)[None, None, None, :] * np.ones((1, n_phi, 1, 1))
    return d.reshape(n_mu * n_phi, n_gauss * n_gauss, 3), wt.reshape(n_mu * n_phi, n_gauss * n_gauss)


def histogram(drv, mat, cos_v, s):
    """The chi-square of the draws s against the reported pdf -> dict of the figures (the caller asserts on them)."""
    d, wt = _grid(N_MU, N_PHI, GAUSS)
    pdf, _val, floored = reported(drv, mat, cos_v, d.reshape(-1, 3))
    expected = N * (pdf.reshape(wt.shape) * wt).sum(axis=1)
    cont = (s["some"] == 1) & ((s["flags"] & 1) == 0)
    dirs = s["dir"][cont].astype(np.float64)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    i = np.minimum(((dirs[:, 2] + 1.0) / 2.0 * N_MU).astype(np.int64), N_MU - 1)
    j = np.minimum((np.mod(np.arctan2(dirs[:, 1], dirs[:, 0]), 2.0 * np.pi) / (2.0 * np.pi) * N_PHI).astype(np.int64), N_PHI - 1)
    observed = np.bincount(i * N_PHI + j, minlength=N_MU * N_PHI).astype(np.float64)
    use = expected >= MIN_EXPECTED
    chi2 = float((((observed - expected) ** 2)[use] / expected[use]).sum())
    dof = int(use.sum())
    return dict(chi2=chi2, dof=dof, p=float(stats.chi2.sf(chi2, dof)), left_out=float(expected[~use].sum() / expected.sum()),
                observed_left_out=float(observed[~use].sum() / max(observed.sum(), 1.0)),
                mass=float(expected.sum() / N), returned=float(cont.mean()), floored_nodes=floored,
                floored_draws=int(((s["pdf"] == FLOOR) & cont).sum()), deltas=int(((s["flags"] & 1) == 1).sum()))


def moment(drv, mat, cos_v, s, n_mu=32, n_phi=64):
    """mean(value * cos / pdf) of the draws and its standard error from 16 blocks of 4096, per channel, against the
    quadrature of eval's value * |cos| on a 256 x 512 grid (32 x 64 cells of 8 x 8 Gauss points) -> (mean [3], se [3],
    quadrature [3])."""
    cont = (s["some"] == 1) & ((s["flags"] & 1) == 0)
    cos = np.abs(s["dir"][:, 2].astype(np.float64))
    wgt = np.where(cont[:, None], s["value"].astype(np.float64) * cos[:, None] / np.where(cont, s["pdf"], 1.0)[:, None], 0.0)
    blocks = wgt.reshape(BLOCKS, -1, 3).mean(axis=1)
    d, wt = _grid(n_mu, n_phi, GAUSS)
    d = d.reshape(-1, 3)
    q = queries(cos_v, len(d))
    q["wi"] = d.astype(np.float32)
    val = drv.eval(mat, q)["value"].astype(np.float64)
    quad = (val * np.abs(d[:, 2:3]) * wt.reshape(-1, 1)).sum(axis=0)
    return blocks.mean(axis=0), blocks.std(axis=0, ddof=1) / np.sqrt(BLOCKS), quad


# ---------------------------------------------------------------- lights ----------------------------------------------------------------
def light_table(records):
    t = np.zeros(len(records), dtype=sc.LIGHT)
    for k, r in enumerate(records):
        for f, v in r.items():
            t[k][f] = v
    return t


def light_draws(drv, table, light, point):
    q = np.zeros(N, dtype=sc.LIGHT_QUERY)
    q["from"] = point
    q["light"] = light
    k = np.arange(N)
    # a 256 x 256 lattice shifted to the cell centres: (u, v) stratified as the integrator's sampler stratifies them
    q["u"] = ((k >> 8) + 0.5) / 256.0
    q["v"] = ((k & 255) + 0.5) / 256.0
    return drv.light_sample(table, q)
