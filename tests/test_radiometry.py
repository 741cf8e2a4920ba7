"""The CPU oracle's integrator against closed-form radiometry (tests/radiometry_ref.py) on the scenes of
tests/radiometry_cases.py: NEE, the MIS weights, the light pick's 1/n_lights, depth truncation, roulette and the
f*cos*cos convention, against values that do not come from the oracle's author. The parity suite compares the device
with the oracle bit for bit; this is what says the oracle (and so the device) computes the right number.
tests/test_gpu_radiometry.py runs the same cases on the device.

Per case and strategy: 16 independent estimates (frame = 0..15 seeds sampler_new) at 64 spp, the mean over pixels and
frames against the truth:  |mean - truth| <= 5 SE + allowance * truth,  SE from the 16 frame means, the allowance from
radiometry_cases.MEASURED (twice the deviation measured at 16 x the samples, at most 2e-3)."""
import numpy as np
import pytest

import radiometry_cases as rc
import radiometry_ref as rr

CASES = {c.name: c for c in rc.cases()}
_means = {}


def frame_means(name, strategy):
    """[16, 3] frame means of one case under one strategy, rendered once for all the tests of this module."""
    if (name, strategy) not in _means:
        _means[name, strategy] = rc.frame_means(rc.oracle_render, CASES[name], strategy, rc.FRAMES)
    return _means[name, strategy]


# ---------------------------------------------------------------- the truth itself ----------------------------------------------------------------
def test_f_avg_diel_is_schlick_f0_not_the_fresnel_average():
    """openpbr.rs:645 scales the diffuse slab by 1 - f0_from_ior(ior). The cosine-weighted average of the exact Fresnel
    reflectance (mpmath quadrature) is more than twice that at ior 1.5; the truth follows the reference's formula."""
    assert rr.f_avg_diel(1.5) == pytest.approx(0.04, abs=1e-15) and rr.f_avg_diel(1.0) == 0.0
    avg = rr.fresnel_average_mp(1.5)
    assert avg == pytest.approx(0.0917780, abs=1e-6)  # the tabulated hemispherical reflectance of glass, 0.092
    assert rr.fresnel_average_mp(1.0) == pytest.approx(0.0, abs=1e-15)
    for ior in (1.1, 1.33, 1.5, 2.0):  # F(mu) >= F0 everywhere, so the average is above F0 for every ior
        assert rr.fresnel_average_mp(ior) > rr.f_avg_diel(ior)


@pytest.mark.parametrize("mu_v,rough,weight", [(0.3, 1.0, 1.0), (0.5, 0.6, 1.0), (0.8, 0.7, 0.0)])
def test_half_vector_rule_matches_adaptive_quadrature(mu_v, rough, weight):
    """The specular lobe's moment by the half-vector rule against scipy's adaptive rule over (cos, phi), where the lobe is
    wide enough for the latter to converge."""
    assert rr.albedo(mu_v, 0.5, 1.5, rough, weight) == pytest.approx(rr.albedo_bruteforce(mu_v, 0.5, 1.5, rough, weight), rel=2e-6)


def test_solid_angles():
    # a unit square seen from its axis at height h: 4 asin(a^2 / (a^2 + h^2)) with a the half side (here 4 asin(1/5))
    o, eu, ev = (-0.5, -0.5, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    assert rr.rect_solid_angle((0, 0, 0), o, eu, ev) == pytest.approx(4.0 * np.arcsin(0.25 / (0.25 + 1.0)), rel=1e-12)
    assert rr.rect_solid_angle((1.3, 0.2, 1.0), o, eu, ev) == 0.0  # in its plane, beside it
    assert rr.rect_solid_angle((0, 0, 1.0 - 1e-9), o, eu, ev) == pytest.approx(2.0 * np.pi, rel=1e-6)  # on it
    assert rr.sphere_cap_solid_angle(2.0, 1.0) == pytest.approx(2.0 * np.pi * (1.0 - np.sqrt(0.75)), rel=1e-14)


def test_light_quadratures_integrate_one_to_the_solid_angle():
    """Both branches of the cone rule and the rectangle rule with fn = 1 against the closed-form solid angles, and with
    fn = l.z^2 / pi against the closed form of a Lambert cone about the normal, 2/3 (1 - cos^3 b)."""
    one = lambda l: 1.0
    b = np.radians(25.0)
    cap = 2.0 * np.pi * (1.0 - np.cos(b))
    assert rr.cone_integral(one, (0.3, -0.2, 0.8), np.cos(b)) == pytest.approx(cap, rel=1e-9)        # above the horizon
    assert rr.cone_integral(one, (0.6, 0.8, 0.0), np.cos(b)) == pytest.approx(cap / 2.0, rel=1e-8)   # halved by it
    assert rr.cone_integral(one, (0.0, 0.0, 1.0), np.cos(b)) == pytest.approx(cap, rel=1e-9)         # about the pole
    wide = np.radians(80.0)  # holds the pole AND is cut by the horizon; with its mirror image it makes the whole cap
    up = rr.cone_integral(one, (np.sin(0.5), 0.0, np.cos(0.5)), np.cos(wide))
    down = rr.cone_integral(one, (np.sin(0.5), 0.0, -np.cos(0.5)), np.cos(wide))
    assert up + down == pytest.approx(2.0 * np.pi * (1.0 - np.cos(wide)), rel=1e-8) and up > down > 0.0
    assert rr.cone_integral(lambda l: l[2] ** 2 / np.pi, (0, 0, 1), np.cos(b)) == pytest.approx(2 / 3 * (1 - np.cos(b) ** 3), rel=1e-9)
    assert rr.cone_integral(one, (0.0, 0.0, -1.0), np.cos(b)) == 0.0                                 # below it
    o, eu, ev = np.array((-0.9, 0.4, 1.5)), np.array((1.0, 0.2, 0.0)), np.array((-0.1, 0.5, 0.3))
    n = np.cross(eu, ev) / np.linalg.norm(np.cross(eu, ev))
    n = -n if n @ o > 0 else n  # facing the origin
    assert rr.rect_integral(one, o, eu, ev, n) == pytest.approx(rr.rect_solid_angle((0, 0, 0), o, eu, ev), rel=1e-9)
    assert rr.rect_integral(one, o, eu, ev, -n) == 0.0  # one-sided



def test_the_interior_recursion_reproduces_the_furnace_gain():
    """The probe that opened this work: a camera at the centre of an emissive sphere (albedo 0.5, Le 1, ior 1.5) sees
    depth 1 on the geometric series Le (1 - a^(d+1)) / (1 - a), a = 0.96 * 0.5 * 2/3, and depths 2 and 3 above it by
    1e-3 and 1.7e-3, more at a low specular_roughness than at 1.0. The recursion over the arrival cosine with the residual
    Schlick lobe (radiometry_ref.slab_f) gives exactly that shape: nothing at normal incidence, a gain per bounce after."""
    a = 0.96 * 0.5 * 2.0 / 3.0
    series = [rr.emissive_sphere_series(d, 1.0, a) for d in (1, 2, 3)]
    assert series == pytest.approx([1.32, 1.4224, 1.455168], abs=1e-12)
    gain = lambda d, rough, ior=1.5: rr.emissive_sphere_interior(d, 1.0, 1.0, 0.5, ior, rough) / rr.emissive_sphere_series(
        d, 1.0, (1.0 - rr.f0_from_ior(ior)) * 0.5 * 2.0 / 3.0) - 1.0
    assert abs(gain(1, 0.05)) < 1e-6
    assert 0.8e-3 < gain(2, 0.05) < 1.6e-3 and 1.3e-3 < gain(3, 0.05) < 2.6e-3 and 2.0e-3 < gain(12, 0.05) < 3.5e-3
    # ior 1.0, where F0 = 0 and the lobe "reflects nothing": the gain follows specular_roughness all the same
    assert 1.0e-3 < gain(2, 0.05, 1.0) < 2.0e-3 and 0.8e-3 < gain(2, 0.3, 1.0) < 1.5e-3 and 0.5e-4 < gain(2, 1.0, 1.0) < 2e-4


def test_the_oracle_shows_the_furnace_gain_and_the_model_explains_it():
    """The same probe on the oracle, camera at the centre, specular_roughness 0.05: depth 1 sits on the geometric series,
    depth 3 stands clear of it, and both sit on the modelled value."""
    centre = rc.camera((0, 0, 0), (0, 0, -1), 10.0)
    a = 0.96 * 0.5 * 2.0 / 3.0
    for depth, off_series in ((1, False), (3, True)):
        case = rc.interior(depth, 0.05)

        def build(strategy, frame, case=case):
            d = case.build(strategy, frame)
            d.camera = centre
            return d

        moved = rc.Case("centre", build, lambda: 0.0)
        m, se = rc.mean_and_se(rc.frame_means(rc.oracle_render, moved, "power", rc.FRAMES))
        series = rr.emissive_sphere_series(depth, 1.0, a)
        model = rr.emissive_sphere_interior(depth, 1.0, 1.0, 0.5, 1.5, 0.05)
        print("depth %d: oracle %.7f +- %.1e, series %.7f, model %.7f" % (depth, m[0], se[0], series, model))
        assert abs(m[0] - model) <= 5.0 * se[0] + 1e-4 * model
        if off_series:
            assert m[0] - series > 5.0 * se[0] and m[0] / series - 1.0 > 1e-3
        else:
            assert abs(m[0] / series - 1.0) < 1e-5


# ---------------------------------------------------------------- the oracle against it ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_matches_the_closed_form(name):
    case = CASES[name]
    truth = case.truth()
    for s in case.strategies:
        allowance = case.allowance(s)
        assert 0.0 < allowance <= 2e-3
        mean, se = rc.mean_and_se(frame_means(name, s))
        print("%s %s: mean %s truth %s rel %+.2e, 5 SE %.2e, allowance %.1e" % (
            name, s, mean, truth, mean[0] / truth[0] - 1.0, 5.0 * se[0] / truth[0], allowance))
        assert np.all(np.abs(mean - truth) <= 5.0 * se + allowance * truth), (name, s, mean, truth, se)


@pytest.mark.parametrize("name", list(CASES))
def test_strategies_agree(name):
    case = CASES[name]
    est = {s: rc.mean_and_se(frame_means(name, s)) for s in case.strategies}
    for i, a in enumerate(case.strategies):
        for b in case.strategies[i + 1:]:
            (ma, sa), (mb, sb) = est[a], est[b]
            assert np.all(np.abs(ma - mb) <= 5.0 * np.sqrt(sa * sa + sb * sb)), (name, a, b, ma, mb, sa, sb)


def test_the_cases_are_the_ones_the_bound_was_measured_for():
    assert set(rc.MEASURED) == set(CASES)
    for n, c in CASES.items():
        assert set(rc.MEASURED[n]) in (set(c.strategies), {"all"}), n
    left_out = {n: c.left_out for n, c in CASES.items() if c.left_out}
    assert left_out == {"distant_0deg": "bsdf: delta-like light", "distant_2deg": "bsdf: delta-like light"}
