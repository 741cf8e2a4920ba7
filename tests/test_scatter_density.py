"""Are the samples distributed with the density the functions report? (tests/scatter_density.py has the method.)
test_eval_matches_scatter_importance checks that scatter and eval report the SAME pdf; nothing checked that the directions
scatter returns HAVE that pdf, nor that sample_li's 1/pdf integrates to the solid angle of the light.

Run here on the oracle and on the device source compiled for the host (the recipe of tests/test_shading_seam_host.py);
tests/test_gpu_scatter_density.py runs the device.

Findings these tests recorded when they were written ("Radiometry"): every lobe's draws pass against its
reported pdf, so the furnace gain is no sampling defect; it is the residual Schlick lobe of specular_weight 0, which the
moment of the Lambert slab shows (it matches radiometry_ref.albedo, which has the lobe, and misses the Lambert value)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import radiometry_ref as rr
import scatter_density as sd
import seam_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(sd.MATERIALS) + list(sd.LAMBERTS)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("density_host") / "libseam_host.so"
    k = os.path.join(ROOT, "crust-render_amd", "csrc", "kernels")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + k,
           os.path.join(ROOT, "tests", "host_shade", "seam_host.cpp"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return sc.Drivers(C.CDLL(str(out)), "host")


@pytest.fixture(scope="module")
def oracle():
    return sc.oracle_drivers()


@pytest.fixture(params=["oracle", "host"])
def drv(request):
    return request.getfixturevalue(request.param)


def check_density(drv, name, cos_v):
    """The assertions of one (material, view) pair, shared with the GPU twin."""
    mat = sd.named(name)
    s = sd.draws(drv, mat, cos_v)
    h = sd.histogram(drv, mat, cos_v, s)
    mean, se, quad = sd.moment(drv, mat, cos_v, s)
    print("%s cos_v %.1f: chi2 %.1f over %d cells p %.3g; left out %.4f of the expected mass (%.4f of the draws); pdf mass "
          "%.5f, returned %.5f; floor reported at %d of %d nodes and by %d draws; moment %.6f +- %.1e, quadrature %.6f"
          % (name, cos_v, h["chi2"], h["dof"], h["p"], h["left_out"], h["observed_left_out"], h["mass"], h["returned"],
             h["floored_nodes"], sd.N_MU * sd.N_PHI * sd.GAUSS ** 2, h["floored_draws"], mean[0], se[0], quad[0]))
    assert h["deltas"] == 0                      # continuous lobes only: a delta sample has no density to test
    assert h["dof"] >= 128 and h["p"] >= sd.P_MIN, h
    assert h["left_out"] <= sd.MAX_LEFT_OUT, h
    # the reported pdf integrates to the fraction of draws that return a sample. The chi-square settles the shape cell
    # by cell; this catches a factor missing from the whole (a pmf, a Jacobian), which is never a matter of under 1 %
    assert abs(h["mass"] - h["returned"]) <= sd.MAX_LEFT_OUT, h
    assert h["floored_draws"] <= sd.N // 1000, h  # the floor is a guard, not a density: hardly a draw may land on it
    if name in sd.LAMBERTS:
        rough, ior = sd.LAMBERTS[name]
        truth = rr.albedo(cos_v, 0.5, ior, rough)
        assert np.all(np.abs(mean - truth) <= 5.0 * se), (name, cos_v, mean, se, truth)
        if rough >= 0.3:  # the grid resolves the residual lobe: eval agrees with the float64 restatement of the slab
            assert np.allclose(quad, truth, rtol=2e-4), (name, cos_v, quad, truth)
    else:
        assert np.all(np.abs(mean - quad) <= 5.0 * se), (name, cos_v, mean, se, quad)
    return s, mean, se


@pytest.mark.parametrize("cos_v", sd.VIEWS)
@pytest.mark.parametrize("name", NAMES)
def test_scatter_draws_have_the_reported_density(drv, oracle, name, cos_v):
    s, _mean, _se = check_density(drv, name, cos_v)
    if drv is not oracle:
        assert len(sc.mismatches(s, sd.draws(oracle, sd.named(name), cos_v))) == 0


def test_the_furnace_gain_is_the_residual_lobe_not_a_sampling_defect(oracle):
    """At cos_v = 0.3 the moment of the "Lambert" slab stands clear of the Lambert value (1 - F0) rho 2/3 and on the
    albedo that includes the Schlick lobe specular_weight 0 leaves; along the normal the two coincide. specular_roughness
    1.0, where the standard error is 1e-5, shows it beyond doubt."""
    mat = sd.lambert(1.0, 1.5)
    lam = 0.96 * 0.5 * 2.0 / 3.0
    for cos_v, gain in ((1.0, False), (0.3, True)):
        mean, se, _quad = sd.moment(oracle, mat, cos_v, sd.draws(oracle, mat, cos_v))
        assert abs(mean[0] - rr.albedo(cos_v, 0.5, 1.5, 1.0)) <= 5.0 * se[0]
        if gain:
            assert mean[0] - lam > 50.0 * se[0] and mean[0] / lam - 1.0 > 5e-3
        else:
            assert abs(mean[0] - lam) <= 5.0 * se[0] + 3e-5 * lam


# ---------------------------------------------------------------- lights ----------------------------------------------------------------
SPHERE = dict(kind=0, geom_id=0, radiance=(3, 3, 3), center=(0.5, 2.0, -0.3), radius=0.7)
RECT = dict(kind=1, geom_id=1, radiance=(3, 3, 3), origin=(-1.0, 1.5, -0.5), edge_u=(2.0, 0.0, 0.0), edge_v=(0.0, 0.0, 1.0),
            normal=(0.0, -1.0, 0.0))
DISTANT = dict(kind=2, geom_id=0xFFFFFFFF, radiance=(2, 2, 2), normal=(0.0, -0.6, 0.8), radius=np.cos(np.radians(10.0)),
               center=(2.0 * np.pi * (1.0 - np.cos(np.radians(10.0))), 0.0, 0.0))
DOME = dict(kind=3, geom_id=0xFFFFFFFF, radiance=(1, 1, 1))
TABLE = sd.light_table([SPHERE, RECT, DISTANT, DOME])
# eight shading points each: the last sphere point stands 5 % of the radius off the surface, the last rectangle point
# lies in the rectangle's plane (beside it), the one before under its edge
SPHERE_POINTS = [(0, 0, 0), (3, 0, 1), (-2, 4, 0), (0.5, -3, -0.3), (4, 2, -0.3), (0.5, 2, 5), (1.5, 2.5, 0.2), (0.5, 2.0 - 0.735, -0.3)]
RECT_POINTS = [(0, 0, 0), (0, 0.5, 0), (3, 0, 2), (-4, 1, 0), (0, 1.4, 0), (0.9, -2, 0.4), (1.0, 0.2, 0.5), (2.5, 1.5, 0.0)]


def check_area_light(drv, light, point, omega):
    """mean(1 / pdf) over a 256 x 256 lattice of sample_li equals the solid angle. solid_angle_pdf (light.rs:180-187) is
    d^2 / (cosine * area + 1e-4), so the mean carries 1e-4 * mean(1 / d^2) more, taken off here; what remains is the
    midpoint rule's error on an integrand with a kink at the silhouette, under (1/256)^2 of the integrand's scale, and
    float32 rounding."""
    s = sd.light_draws(drv, TABLE, light, point)
    assert s["some"].all()
    inv = 1.0 / s["pdf"].astype(np.float64)
    d2 = s["distance"].astype(np.float64) ** 2
    got = float(np.mean(inv - 1e-4 / d2))
    print("light %d from %s: mean(1/pdf) %.7f, solid angle %.7f" % (light, point, got, omega))
    assert abs(got - omega) <= 1e-4 * max(omega, float(np.max(inv))), (light, point, got, omega)
    return s


@pytest.mark.parametrize("point", SPHERE_POINTS)
def test_sphere_light_pdf_integrates_to_the_cap(drv, point):
    d = np.linalg.norm(np.array(SPHERE["center"]) - np.array(point, np.float64))
    check_area_light(drv, 0, point, rr.sphere_cap_solid_angle(d, SPHERE["radius"]))


@pytest.mark.parametrize("point", RECT_POINTS)
def test_rect_light_pdf_integrates_to_its_solid_angle(drv, point):
    omega = rr.rect_solid_angle(point, RECT["origin"], RECT["edge_u"], RECT["edge_v"])
    # the rectangle emits along -y only: a point above its plane sees the dark side, and sample_li says so with pdf -> inf
    check_area_light(drv, 1, point, omega if point[1] < RECT["origin"][1] else 0.0)


def uniform_chi2(dirs, axis, cos_min):
    """Pearson's chi-square of unit directions against the uniform density over the cap of cosines [cos_min, 1] about
    `axis`, on 16 x 32 equal-area cells -> (p, directions outside the cap)."""
    axis = np.asarray(axis, np.float64)
    e1 = np.cross(axis, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(axis, e1)
    c = dirs @ axis
    phi = np.mod(np.arctan2(dirs @ e2, dirs @ e1), 2.0 * np.pi)
    outside = int((c < cos_min - 1e-6).sum())
    i = np.clip(((c - cos_min) / (1.0 - cos_min) * 16).astype(np.int64), 0, 15)
    j = np.minimum((phi / (2.0 * np.pi) * 32).astype(np.int64), 31)
    observed = np.bincount(i * 32 + j, minlength=512).astype(np.float64)
    expected = len(dirs) / 512.0
    return float(sd.stats.chi2.sf(((observed - expected) ** 2 / expected).sum(), 512)), outside


def test_distant_and_dome_lights_sample_their_constant_pdf(drv):
    """pdf = 1 / Omega for both (light.rs:285-303, :358-388), and the directions are uniform over the cone / the sphere."""
    s = sd.light_draws(drv, TABLE, 2, (1.0, 2.0, 3.0))
    omega = 2.0 * np.pi * (1.0 - np.cos(np.radians(10.0)))
    assert np.allclose(s["pdf"], 1.0 / omega, rtol=1e-6) and np.isinf(s["distance"]).all()
    p, outside = uniform_chi2(s["direction"].astype(np.float64), -np.array(DISTANT["normal"]), np.cos(np.radians(10.0)))
    assert p >= sd.P_MIN and outside == 0, (p, outside)
    s = sd.light_draws(drv, TABLE, 3, (1.0, 2.0, 3.0))
    assert np.allclose(s["pdf"], 1.0 / (4.0 * np.pi), rtol=1e-6)
    p, outside = uniform_chi2(s["direction"].astype(np.float64), np.array([0.0, 1.0, 0.0]), -1.0)
    assert p >= sd.P_MIN and outside == 0, (p, outside)
    # the test has teeth: the same directions against a cone 10 % narrower fail it
    assert uniform_chi2(sd.light_draws(drv, TABLE, 2, (0, 0, 0))["direction"].astype(np.float64), -np.array(DISTANT["normal"]),
                        np.cos(np.radians(9.0)))[0] < sd.P_MIN
