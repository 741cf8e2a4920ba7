"""The CPU oracle's carried interior medium against closed forms (tests/media_ref.py) on the scenes of
tests/media_cases.py: Beer-Lambert along a chord, the free-flight competition under the majorant, the chromatic weights,
the Henyey-Greenstein bounce as the integrator uses it and the transmittance of the depth-exhausted arm, against values
that do not come from the oracle's author. tests/test_gpu_media.py runs the same cases on the device.

Per case and strategy: 16 independent estimates (frame = 0..15 seeds sampler_new) at the case's samples, the mean over
pixels and frames against the truth:  |mean - truth| <= 5 SE + allowance * truth,  SE from the 16 frame means, the
allowance from media_cases.MEASURED (twice the deviation measured at 16 x the samples, at most 2e-3)."""
import numpy as np
import pytest
from scipy import integrate

import media_cases as mc
import media_ref as mr

CASES = {c.name: c for c in mc.cases()}
_means = {}


def frame_means(case, strategy):
    """[16, n] frame means of one case under one strategy, rendered once for all the tests of this module."""
    if (case.name, strategy) not in _means:
        _means[case.name, strategy] = mc.frame_means(mc.oracle_render, case, strategy, mc.FRAMES)
    return _means[case.name, strategy]


# ---------------------------------------------------------------- the truth itself ----------------------------------------------------------------
def test_medium_from_transmission():
    a, s, g = mr.medium_from_transmission((0.8, 0.5, 0.2), 2.0)
    assert a == pytest.approx(-np.log([0.8, 0.5, 0.2]) / 2.0, rel=1e-15) and not s.any() and g == 0.0
    a, _s, _g = mr.medium_from_transmission((0.0, 1.0, 2.0), 1.0)  # the tint is clamped to [1e-4, 1]
    assert a == pytest.approx([-np.log(1e-4), 0.0, 0.0], abs=1e-15)
    # scatter above the extinction on one channel: sigma_a is shifted up on all three, sigma_s stays
    a, s, g = mr.medium_from_transmission((0.5, 0.5, 0.5), 1.0, (1.0, 0.2, 0.0), 5.0)
    assert s == pytest.approx([1.0, 0.2, 0.0]) and a == pytest.approx([0.0, 0.8, 1.0], abs=1e-15) and g == 0.999
    assert mr.sigma_t((a, s, g)) == pytest.approx([1.0, 1.0, 1.0])  # the shift raises sigma_t above -ln(tint) / depth
    assert not any(x.any() for x in mr.medium_from_transmission((0.5, 0.5, 0.5), 0.0)[:2])  # depth 0: no medium


def test_medium_from_subsurface_and_blend():
    a, s, g = mr.medium_from_subsurface((0.0, 0.5, 1.0), 2.0, (1.0, 0.5, 1e-9), 0.3)
    assert a + s == pytest.approx([0.5, 1.0, 1000.0]) and g == 0.3  # 1 / max(radius * scale, 1e-3)
    alpha = s / (a + s)
    assert alpha[0] == pytest.approx(0.0, abs=1e-5) and alpha[2] == pytest.approx(1.0, abs=1e-5) and 0.9 < alpha[1] < 1.0
    sv = 4.09712 + 4.20863 * 0.5 - np.sqrt(9.59217 + 41.6808 * 0.5 + 17.7126 * 0.25)
    assert alpha[1] == pytest.approx((1 - sv * sv) / (1 - 0.3 * sv * sv), rel=1e-14)
    m1, m2 = (np.array([1.0, 2.0, 3.0]), np.zeros(3), 0.7), (np.array([0.5, 0.5, 0.5]), np.array([3.0, 3.0, 3.0]), -0.2)
    ba, bs, bg = mr.medium_blend(m1, 0.75, m2, 0.25)
    assert ba == pytest.approx([0.875, 1.625, 2.375]) and bs == pytest.approx([0.75] * 3) and bg == pytest.approx(-0.2)
    assert mr.medium_blend(m1, 0.5, m1, 0.5)[2] == 0.0  # nothing scatters: g 0
    # interior_medium: the weights are t and (1 - t) * subsurface_weight over their sum; no weight or no extinction: none
    mat = mc.glass((0.6, 0.5, 0.45), 1.0, transmission_weight=0.6, subsurface_weight=0.5, subsurface_color=(0.5,) * 3,
                   subsurface_radius=1.0, subsurface_radius_scale=(1.0, 0.9, 0.8))
    med = mr.interior_medium(mat)
    sub = mr.medium_from_subsurface((0.5,) * 3, 1.0, (1.0, 0.9, 0.8))
    assert mr.sigma_t(med) == pytest.approx(0.75 * -np.log([0.6, 0.5, 0.45]) + 0.25 * mr.sigma_t(sub), rel=1e-14)
    assert mr.is_scattering(med) and mr.sigma_t(med).min() > 0.55 * mr.sigma_t(med).max()
    assert mr.interior_medium({"transmission_weight": 0.0}) is None
    assert mr.interior_medium({"transmission_weight": 1.0, "transmission_depth": 1.0}) is None  # white tint


def test_fresnel_and_snell():
    assert mr.fresnel_dielectric(1.0, 1.0, 1.5) == pytest.approx(0.04, abs=1e-15) == mr.f0_from_ior(1.5)
    assert mr.fresnel_dielectric(1.0, 1.5, 1.0) == pytest.approx(0.04, abs=1e-15)
    assert mr.snell(0.8, 1.0, 1.5) == pytest.approx(np.sqrt(1.0 - 0.36 / 2.25), rel=1e-15)
    critical = np.sqrt(1.0 - 1.0 / 2.25)
    assert mr.snell(critical - 1e-9, 1.5, 1.0) is None and mr.fresnel_dielectric(critical - 1e-9, 1.5, 1.0) == 1.0
    assert mr.snell(critical + 1e-9, 1.5, 1.0) is not None
    brewster = np.cos(np.arctan(1.5))  # r_par vanishes: F is half of r_perp^2
    ct = mr.snell(brewster, 1.0, 1.5)
    assert mr.fresnel_dielectric(brewster, 1.0, 1.5) == pytest.approx(0.5 * ((brewster - 1.5 * ct) / (brewster + 1.5 * ct)) ** 2, rel=1e-12)
    # reciprocity: the same reflectance from either side along one refracted path
    assert mr.fresnel_dielectric(0.8, 1.0, 1.5) == pytest.approx(mr.fresnel_dielectric(mr.snell(0.8, 1.0, 1.5), 1.5, 1.0), rel=1e-13)
    assert mr.schlick(1.0, 0.04) == 0.04 and mr.schlick(0.0, 0.04) == 1.0 and mr.reflection_factor(0.5, 1.5) == pytest.approx(0.5 * (0.04 + 0.96 / 32))


@pytest.mark.parametrize("cos_v,eta_i,eta_t", [(0.8, 1.0, 1.5), (0.9, 1.5, 1.0)])
def test_the_stated_btdf_conserves_flux_and_carries_no_eta_squared(cos_v, eta_i, eta_t):
    """openpbr.rs:862-914 integrated over l as it stands (alpha 0.3, where adaptive quadrature converges) equals the
    half-vector form in which eta_t^2 has cancelled against the Jacobian, and that form tends to 1 - F at the alpha of the
    test scenes: one passage is (1 - F) cos, not (eta_t / eta_i)^2 (1 - F) cos."""
    assert mr.btdf_albedo(cos_v, eta_i, eta_t, 0.3, 1e-6) == pytest.approx(mr.btdf_albedo_over_h(cos_v, eta_i, eta_t, 0.3, 1e-8), rel=1e-6)
    smooth = mr.btdf_albedo_over_h(cos_v, eta_i, eta_t, 1e-4)
    assert smooth == pytest.approx(1.0 - mr.fresnel_dielectric(cos_v, eta_i, eta_t), rel=1e-6)
    assert smooth * mr.snell(cos_v, eta_i, eta_t) == pytest.approx(mr.interface_factor(cos_v, eta_i, eta_t), rel=1e-6)


@pytest.mark.parametrize("g", [-0.6, 0.0, 0.6, 0.95])
def test_hg_is_a_density_with_mean_cosine_g_about_the_direction_of_travel(g):
    one = integrate.quad(lambda mu: 2.0 * np.pi * mr.hg_phase(mu, g), -1.0, 1.0, epsabs=1e-12)[0]
    mean = integrate.quad(lambda mu: 2.0 * np.pi * mr.hg_phase(mu, g) * mu, -1.0, 1.0, epsabs=1e-12)[0]
    assert one == pytest.approx(1.0, abs=1e-10) and mean == pytest.approx(g, abs=1e-10)
    # the sampling rule of medium.rs:158-184 inverts this density's distribution function: u1 = P(mu' <= mu)
    if g:
        for u1 in (0.1, 0.5, 0.9):
            sq = (1.0 - g * g) / (1.0 - g + 2.0 * g * u1)
            mu = (1.0 + g * g - sq * sq) / (2.0 * g)
            assert integrate.quad(lambda m: 2.0 * np.pi * mr.hg_phase(m, g), -1.0, mu, epsabs=1e-12)[0] == pytest.approx(u1, abs=1e-9)


def test_single_scatter_quadrature():
    sig_t, sig_s, d = 0.7, 0.45, 1.0
    assert mr.single_scatter_slab(1.5, sig_t, 1e-12, 0.0, d) < 1e-12  # sigma_s -> 0: it vanishes
    assert mr.single_scatter_slab(1.5, sig_t, sig_s, 0.0, d, interface=False) == pytest.approx(mr.single_scatter_e2(sig_t, sig_s, d), abs=1e-9)
    # the collision depth integrated in closed form: e^{-sigma_t d / mu} (e^{k d} - 1) / k, k = sigma_t (1 / mu - 1)
    for g in (-0.6, 0.0, 0.6):
        def over_mu(mu):
            k = sig_t * (1.0 / mu - 1.0)
            inner = np.exp(-sig_t * d / mu) * (np.expm1(k * d) / k if k > 1e-12 else d)
            return sig_s * 2.0 * np.pi * mr.hg_phase(mu, g) * inner * mr.interface_factor(mu, 1.5, 1.0)
        want = 0.96 * integrate.quad(over_mu, np.sqrt(1.0 - 1.0 / 2.25), 1.0, epsabs=1e-13, epsrel=1e-12)[0]
        assert mr.single_scatter_slab(1.5, sig_t, sig_s, g, d) == pytest.approx(want, abs=1e-9)


def test_the_three_anisotropies_stand_far_apart():
    """A flipped phase direction would swap g = -0.6 and +0.6: their truths differ by 50 times the widest bound."""
    t = {g: CASES["single_scatter_g%+.1f" % g].truth() for g in mc.SINGLE_G}
    for a, b in ((-0.6, 0.0), (0.0, 0.6)):
        assert np.all(t[b] - t[a] > 0.02 * t[b]), (a, b, t[a], t[b])  # the bound is 5 SE + allowance <= 1.2 %
    assert np.all(t[0.6] - t[-0.6] > 0.1 * t[0.6])


def test_the_variance_condition_holds_in_every_scattering_case():
    assert mr.scatter_weight_second_moment(0.5, 0.5, 1.0) == np.inf and mr.scatter_weight_second_moment(1.0, 1.0, 1.0) == 1.0
    mats = [mc.glass(mc.SCATTER_TINT, 1.0, mc.SCATTER),
            mc.glass(mc.CONSERVATIVE_TINT, mc.CONSERVATIVE_DEPTH, tuple(-np.log(mc.CONSERVATIVE_TINT)))]
    for m in mats:
        s = mr.sigma_t(mr.interior_medium(m))
        assert s.min() > 0.55 * s.max(), s
    sa, ss, _g = mr.interior_medium(mats[1])
    assert np.abs(sa).max() < 1e-15 and ss == pytest.approx(-np.log(mc.CONSERVATIVE_TINT) / mc.CONSERVATIVE_DEPTH)


# ---------------------------------------------------------------- the oracle against it ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_matches_the_closed_form(name):
    case = CASES[name]
    truth = case.truth()
    for s in case.strategies:
        allowance = case.allowance(s)
        assert 0.0 < allowance <= 2e-3
        mean, se = mc.mean_and_se(frame_means(case, s))
        print("%s %s: mean %s truth %s rel %s, 5 SE %.2e, allowance %.1e" % (
            name, s, mean, truth, mean / truth - 1.0, 5.0 * (se / truth).max(), allowance))
        assert np.all(5.0 * se < 0.01 * truth), (name, s, se / truth)  # the samples were chosen for this
        assert np.all(np.abs(mean - truth) <= 5.0 * se + allowance * truth), (name, s, mean, truth, se)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.lit])
def test_strategies_agree(name):
    case = CASES[name]
    est = {s: mc.mean_and_se(frame_means(case, s)) for s in case.strategies}
    for i, a in enumerate(case.strategies):
        for b in case.strategies[i + 1:]:
            (ma, sa), (mb, sb) = est[a], est[b]
            assert np.all(np.abs(ma - mb) <= 5.0 * np.sqrt(sa * sa + sb * sb)), (name, a, b, ma, mb, sa, sb)


@pytest.mark.parametrize("form", mc.FORMS)
def test_depth_1_is_exactly_black(form):
    """max_depth 1 ends the path inside the glass: no pixel sees the wall."""
    case = mc.clear_slab(1.0, 1, form)
    for s in case.strategies:
        assert not np.asarray(mc.oracle_render(case.build(s, 0), mc.rc.SPP)).any()


@pytest.mark.parametrize("depth", [3, 8])
def test_chromatic_weights_agree_with_the_grey_render(depth):
    """A conservative slab with sigma_t = (1.39, 1.83, 2.41): channel c against the grey slab of that channel's sigma_t,
    within 5 sqrt(SE_a^2 + SE_b^2). The grey run's weights are all 1 (sigma_bar = sigma_t), the chromatic run's are
    sigma_s / sigma_bar e^{(sigma_bar - sigma_t) t} at a collision and e^{(sigma_bar - sigma_t) t} at a surface; depth 8
    brings multiple scattering and the roulette."""
    chroma, greys = mc.chromatic_vs_grey(depth)
    mean, se = mc.mean_and_se(frame_means(chroma, "power"))
    for c, grey in enumerate(greys):
        gm, gs = mc.mean_and_se(frame_means(grey, "power"))
        assert gm[0] == gm[1] == gm[2] and gm[0] > 0.05
        print("depth %d channel %d: chromatic %.6f +- %.1e, grey %.6f +- %.1e" % (depth, c, mean[c], se[c], gm[c], gs[c]))
        assert 5.0 * np.hypot(se[c], gs[c]) < 0.05 * gm[c]
        assert abs(mean[c] - gm[c]) <= 5.0 * np.hypot(se[c], gs[c]), (depth, c, mean[c], gm[c], se[c], gs[c])


def test_the_cases_are_the_ones_the_bound_was_measured_for():
    assert set(mc.MEASURED) == set(CASES)
    for n, c in CASES.items():
        assert set(mc.MEASURED[n]) == (set(c.strategies) if c.lit else {"all"}), n
        assert c.spp % 64 == 0 and c.spp <= 1024
