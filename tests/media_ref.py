"""Closed-form truth for the carried interior medium: what a pixel is under the reference's STATED model of glass with
an absorbing or scattering interior, in float64, with no dependence on oracle/ or on the product. tests/test_media.py
holds the CPU oracle against these values, tests/test_gpu_media.py the device. The model is stated, not corrected.

The medium (medium.rs:40-114, openpbr.rs:225-258)
  from_transmission  sigma_t = -ln(clamp(tint, 1e-4, 1)) / depth,  sigma_s = max(scatter, 0) / depth,  sigma_a = sigma_t -
                     sigma_s, and where a channel of sigma_a comes out negative the smallest channel is subtracted from
                     all three (sigma_a is SHIFTED up, so sigma_t grows); depth <= 1e-6 gives no medium.
  from_subsurface    sigma_t = 1 / max(radius * radius_scale, 1e-3), sigma_s = sigma_t * alpha_ss(albedo, g) by the
                     van de Hulst inversion  s = 4.09712 + 4.20863 a - sqrt(9.59217 + 41.6808 a + 17.7126 a^2),
                     alpha_ss = clamp((1 - s^2) / (1 - g s^2), 0, 1).
  blend              the sigma's by the weights t = transmission_weight, (1 - t) * subsurface_weight over their sum, g by
                     the mean scattering of each side.

The interface (openpbr.rs:862-949, :1026-1072; brdf.rs:230-240, :10-12)
  The transmission lobe is Walter's GGX BTDF (his eq. 21) at max(specular_roughness, 0.01),
        f_t = (v.h)(-l.h) / ((n.v)(n.l)) * eta_t^2 (1 - F(v.h)) D G2 / (eta_i v.h + eta_t l.h)^2,
  times transmission_weight (times transmission_color when transmission_depth is 0: otherwise the medium owns the
  colour). With d(omega_h) / d(omega_l) = eta_t^2 |l.h| / (eta_i v.h + eta_t l.h)^2 (his eq. 17) the eta_t^2 of the value
  is the Jacobian's and cancels:  integral f_t |cos theta_l| d(omega_l) = integral (v.h) / (n.v) (1 - F) G2 D d(omega_h),
  which is 1 - F in the smooth limit (btdf_albedo below integrates the stated f_t). The lobe conserves flux; it carries NO
  (eta_t / eta_i)^2 radiance scaling. Material::scatter returns f |cos theta_l| and the tracer multiplies by |cos theta_l|
  once more (the cos^2 convention of DESIGN.md "Radiometry"), so one smooth passage of an interface multiplies the path by
        w * (1 - F(theta_i)) * |cos theta_l|,            F the exact dielectric Fresnel, theta_l the refracted angle.
  Entering and leaving a slab:  w^2 (1 - F)^2 cos theta_t cos theta_i  (the exit angle in air is the entry angle). An
  emitter INSIDE the glass is seen at (1 - F) cos theta_t of its radiance, not at eta^2 times that.
  The reflection lobe is GGX with SCHLICK's Fresnel at F0 = ((ior - 1) / (ior + 1))^2, inside the glass as outside (no
  total internal reflection in it); by the same convention one reflection multiplies by F_schlick(cos) * cos.
  A reflected ray is built WITHOUT a medium (openpbr.rs:1131: Ray::new), so after an internal reflection the path is no
  longer attenuated: the echo series below carries ONE passage of absorption whatever the number of reflections.

Unscattered term of a slab of thickness d in front of a wall of radiance L:
        L * w^2 (1 - F(theta_i))^2 cos theta_t cos theta_i exp(-sigma_t d / cos theta_t)                 max_depth >= 2
Echo (normal incidence, R = F0 * 1): the path enter, k pairs of internal reflections, leave, has 2 + 2k vertices:
        L * (1 - F0)^2 exp(-sigma_t d) * sum_{k=0}^{floor((max_depth - 2) / 2)} R^(2k)
Sphere of radius R: a ray entering under theta_t runs the chord 2 R cos theta_t and meets the far side under theta_t.
Single scatter: single_scatter_slab below."""
import numpy as np
from scipy import integrate, special

PI = np.pi
QUAD_TOL = 1e-11


# ---------------------------------------------------------------- the medium ----------------------------------------------------------------
def medium_from_transmission(tint, depth, scatter=(0.0, 0.0, 0.0), g=0.0):
    """medium.rs:40-66 -> (sigma_a, sigma_s, g)."""
    if depth <= 1e-6:
        return np.zeros(3), np.zeros(3), 0.0
    t = np.clip(np.asarray(tint, np.float64), 1e-4, 1.0)
    extinction = -np.log(t) / depth
    sigma_s = np.maximum(np.asarray(scatter, np.float64), 0.0) / depth
    sigma_a = extinction - sigma_s
    if sigma_a.min() < 0.0:
        sigma_a = sigma_a - sigma_a.min()
    return sigma_a, sigma_s, float(np.clip(g, -0.999, 0.999))


def medium_from_subsurface(albedo, radius, radius_scale, g=0.0):
    """medium.rs:77-97 -> (sigma_a, sigma_s, g)."""
    mfp = np.maximum(radius * np.asarray(radius_scale, np.float64), 1e-3)
    sigma_t = 1.0 / mfp
    g = float(np.clip(g, -0.999, 0.999))
    a = np.clip(np.asarray(albedo, np.float64), 0.0, 1.0)
    s = 4.09712 + 4.20863 * a - np.sqrt(9.59217 + 41.6808 * a + 17.7126 * a * a)
    alpha_ss = np.clip((1.0 - s * s) / (1.0 - g * s * s), 0.0, 1.0)
    return sigma_t * (1.0 - alpha_ss), sigma_t * alpha_ss, g


def medium_blend(a, wa, b, wb):
    """medium.rs:103-114."""
    sa, sb = a[1].mean() * wa, b[1].mean() * wb
    g = (a[2] * sa + b[2] * sb) / (sa + sb) if sa + sb > 1e-8 else 0.0
    return a[0] * wa + b[0] * wb, a[1] * wa + b[1] * wb, g


def interior_medium(m):
    """openpbr.rs:225-258 on a material dict with the reference's defaults -> (sigma_a, sigma_s, g) or None."""
    get = lambda k, default: m.get(k, default)
    t = float(get("transmission_weight", 0.0))
    sss = (1.0 - t) * float(get("subsurface_weight", 0.0))
    if t + sss <= 0.0:
        return None
    med = medium_from_transmission(get("transmission_color", (1, 1, 1)), float(get("transmission_depth", 0.0)),
                                   get("transmission_scatter", (0, 0, 0)), float(get("transmission_scatter_anisotropy", 0.0)))
    if sss > 0.0:
        sub = medium_from_subsurface(get("subsurface_color", (0.8, 0.8, 0.8)), float(get("subsurface_radius", 1.0)),
                                     get("subsurface_radius_scale", (1.0, 0.5, 0.25)), float(get("subsurface_scatter_anisotropy", 0.0)))
        med = medium_blend(med, t / (t + sss), sub, sss / (t + sss))
    return None if (med[0] + med[1]).max() <= 1e-6 else med


def sigma_t(med):
    return med[0] + med[1]


def is_scattering(med):
    return med[1].max() > 1e-6


# ---------------------------------------------------------------- the interface ----------------------------------------------------------------
def f0_from_ior(ior):
    return ((ior - 1.0) / (ior + 1.0)) ** 2


def schlick(cos, f0):  # brdf.rs:10-12
    return f0 + (1.0 - f0) * (1.0 - cos) ** 5


def snell(cos_i, eta_i, eta_t):
    """Cosine of the refracted direction, or None under total internal reflection."""
    sin2_t = (eta_i / eta_t) ** 2 * (1.0 - cos_i * cos_i)
    return None if sin2_t >= 1.0 else float(np.sqrt(1.0 - sin2_t))


def fresnel_dielectric(cos_i, eta_i, eta_t):  # brdf.rs:230-240
    cos_i = min(max(cos_i, 0.0), 1.0)
    cos_t = snell(cos_i, eta_i, eta_t)
    if cos_t is None:
        return 1.0
    r_par = (eta_t * cos_i - eta_i * cos_t) / (eta_t * cos_i + eta_i * cos_t)
    r_perp = (eta_i * cos_i - eta_t * cos_t) / (eta_i * cos_i + eta_t * cos_t)
    return 0.5 * (r_par * r_par + r_perp * r_perp)


def interface_factor(cos_i, eta_i, eta_t, weight=1.0):
    """One smooth passage under the cos^2 convention: weight (1 - F) |cos theta_l|; 0 under total internal reflection."""
    cos_t = snell(cos_i, eta_i, eta_t)
    if cos_t is None:
        return 0.0
    return weight * (1.0 - fresnel_dielectric(cos_i, eta_i, eta_t)) * cos_t


def reflection_factor(cos_i, ior):
    """One smooth reflection under the same convention: F_schlick(cos) * cos."""
    return schlick(cos_i, f0_from_ior(ior)) * cos_i


def _ggx_d(hz, a):
    t = (1.0 - hz * hz) / (a * a) + hz * hz
    return 1.0 / (PI * a * a * t * t)


def _ggx_lambda(wz, a):
    return 0.5 * (-1.0 + np.sqrt(1.0 + a * a * (1.0 - wz * wz) / max(wz * wz, 1e-300)))


def btdf(v, l, eta_i, eta_t, alpha):
    """openpbr.rs:862-914 at isotropic alpha, in the ray-facing frame (v.z > 0 > l.z): the stated f_t, without a cosine."""
    h = -(eta_i * v + eta_t * l)
    if h @ h < 1e-24:
        return 0.0
    h = h / np.linalg.norm(h)
    h = -h if h[2] < 0.0 else h
    vh, lh = v @ h, l @ h
    if vh <= 0.0 or lh >= 0.0:
        return 0.0
    g2 = 1.0 / (1.0 + _ggx_lambda(v[2], alpha) + _ggx_lambda(l[2], alpha))
    denom = eta_i * vh + eta_t * lh
    return vh * -lh / (v[2] * -l[2]) * eta_t * eta_t * (1.0 - fresnel_dielectric(vh, eta_i, eta_t)) * _ggx_d(h[2], alpha) * g2 / (denom * denom)


def btdf_albedo(cos_v, eta_i, eta_t, alpha, tol=1e-7):
    """integral f_t |cos theta_l| d(omega_l) over the far hemisphere, by adaptive quadrature of the stated f_t over l."""
    v = np.array([np.sqrt(1.0 - cos_v * cos_v), 0.0, cos_v])

    def g(phi, c):
        s = np.sqrt(1.0 - c * c)
        return btdf(v, np.array([s * np.cos(phi), s * np.sin(phi), -c]), eta_i, eta_t, alpha) * c

    return 2.0 * integrate.dblquad(g, 0.0, 1.0, 0.0, PI, epsabs=tol, epsrel=tol)[0]


def btdf_albedo_over_h(cos_v, eta_i, eta_t, alpha, tol=1e-9):
    """The same integral after the change of variables of the docstring: integral (v.h) / (n.v) (1 - F) G2 D d(omega_h).
    With tan^2(theta_h) = alpha^2 u / (1 - u), D h.z d(omega_h) = du dphi / (2 pi): smooth down to alpha = 1e-4."""
    v = np.array([np.sqrt(1.0 - cos_v * cos_v), 0.0, cos_v])
    rel = eta_i / eta_t

    def g(phi, u):
        t2 = alpha * alpha * u / (1.0 - u)
        hz = 1.0 / np.sqrt(1.0 + t2)
        hs = np.sqrt(t2) * hz
        h = np.array([hs * np.cos(phi), hs * np.sin(phi), hz])
        vh = v @ h
        sin2 = rel * rel * (1.0 - vh * vh)
        if vh <= 0.0 or sin2 >= 1.0:
            return 0.0
        l = -rel * v + (rel * vh - np.sqrt(1.0 - sin2)) * h
        if l[2] >= 0.0:
            return 0.0
        g2 = 1.0 / (1.0 + _ggx_lambda(v[2], alpha) + _ggx_lambda(l[2], alpha))
        return vh / v[2] * (1.0 - fresnel_dielectric(vh, eta_i, eta_t)) * g2 / hz / (2.0 * PI)

    return 2.0 * integrate.dblquad(g, 0.0, 1.0 - 1e-12, 0.0, PI, epsabs=tol, epsrel=tol)[0]


# ---------------------------------------------------------------- Henyey-Greenstein ----------------------------------------------------------------
def hg_phase(mu, g):
    """medium.rs:148-184: density per solid angle of the cosine mu between the direction of TRAVEL before the collision and
    the direction after it; g > 0 scatters forward (sample_henyey_greenstein maps u1 = 1 to mu = +1 about wi = ray.dir)."""
    return (1.0 - g * g) / (4.0 * PI * (1.0 + g * g - 2.0 * g * mu) ** 1.5)


# ---------------------------------------------------------------- closed forms ----------------------------------------------------------------
def slab_unscattered(cos_i, ior, sig_t, d, weight=1.0):
    """Wall radiance 1 seen through a slab of thickness d under the entry cosine cos_i (see the module docstring)."""
    cos_t = snell(cos_i, 1.0, ior)
    through = interface_factor(cos_i, 1.0, ior, weight) * interface_factor(cos_t, ior, 1.0, weight)
    return through * np.exp(-np.asarray(sig_t, np.float64) * d / cos_t)


def slab_echo_normal(max_depth, ior, sig_t, d, weight=1.0):
    """Normal incidence, clear medium: the unscattered term times the echo series in max_depth. Every reflected ray has lost
    the medium, so the absorption is paid once."""
    if max_depth < 2:
        return np.zeros(3)
    r = reflection_factor(1.0, ior)
    return slab_unscattered(1.0, ior, sig_t, d, weight) * sum(r ** (2 * k) for k in range((max_depth - 2) // 2 + 1))


def sphere_chord(radius, cos_t):
    return 2.0 * radius * cos_t


def ball_depth2(cos_i, ior, sig_t, radius, shell_radiance=1.0):
    """A glass ball inside an emissive shell, max_depth 2: through the ball (chord 2 R cos theta_t, the far side met under
    theta_t, left under theta_i) plus the first vertex's mirror reflection, which sees the shell too."""
    cos_t = snell(cos_i, 1.0, ior)
    through = interface_factor(cos_i, 1.0, ior) * interface_factor(cos_t, ior, 1.0)
    return shell_radiance * (through * np.exp(-np.asarray(sig_t, np.float64) * sphere_chord(radius, cos_t)) + reflection_factor(cos_i, ior))


def embedded_emitter(cos_i, ior, sig_t, s0, emission=1.0, weight=1.0):
    """An emitter inside the glass at depth s0 below the front face: (1 - F) cos theta_t exp(-sigma_t s0 / cos theta_t)."""
    cos_t = snell(cos_i, 1.0, ior)
    return emission * interface_factor(cos_i, 1.0, ior, weight) * np.exp(-np.asarray(sig_t, np.float64) * s0 / cos_t)


def single_scatter_slab(ior, sig_t, sig_s, g, d, interface=True):
    """Once-scattered radiance through a laterally infinite slab at normal incidence, per unit wall radiance, one channel.
    The ray enters (entry factor 1 - F0), collides at depth s with density sigma_s exp(-sigma_t s), turns by the
    cosine mu with density 2 pi p_HG(mu), runs (d - s) / mu to the back face and leaves it under cos_out =
    sqrt(1 - eta^2 (1 - mu^2)) with the factor (1 - F(mu)) cos_out; mu runs over (mu_tir, 1], mu_tir =
    sqrt(1 - 1 / eta^2). interface=False replaces every interface factor by 1 and lets mu run over (0, 1]."""
    def exit_factor(mu):
        return interface_factor(mu, ior, 1.0) if interface else 1.0

    def integrand(s, mu):
        return sig_s * np.exp(-sig_t * s) * 2.0 * PI * hg_phase(mu, g) * np.exp(-sig_t * (d - s) / mu) * exit_factor(mu)

    mu_lo = np.sqrt(1.0 - 1.0 / (ior * ior)) if interface else 0.0
    val = integrate.dblquad(integrand, mu_lo, 1.0, 0.0, d, epsabs=QUAD_TOL, epsrel=1e-10)[0]
    return (interface_factor(1.0, 1.0, ior) if interface else 1.0) * val


def single_scatter_e2(sig_t, sig_s, d):
    """The textbook isotropic single scatter of a bare slab: sigma_s / 2 * integral_0^d exp(-sigma_t s) E2(sigma_t (d - s)) ds."""
    return integrate.quad(lambda s: 0.5 * sig_s * np.exp(-sig_t * s) * special.expn(2, sig_t * (d - s)), 0.0, d,
                          epsabs=QUAD_TOL, epsrel=1e-12)[0]


def scatter_weight_second_moment(sig_t, sig_s, sig_bar):
    """E[w^2] of the scatter weight (sigma_s / sigma_bar) e^{(sigma_bar - sigma_t) t}, t ~ Exp(sigma_bar), in an infinite
    medium: (sigma_s / sigma_bar)^2 sigma_bar / (2 sigma_t - sigma_bar), infinite where sigma_t <= sigma_bar / 2."""
    return np.inf if 2.0 * sig_t <= sig_bar else (sig_s / sig_bar) ** 2 * sig_bar / (2.0 * sig_t - sig_bar)
