"""Closed-form radiometry for the integrator tests: the expectation of a pixel under the reference's STATED estimator,
in float64, with no dependence on oracle/ or on the product. tests/test_radiometry.py holds the oracle against these
values, tests/test_gpu_radiometry.py the device.

Two conventions of the reference are part of the estimator and therefore of the truth:
  * Material::eval / scatter return f*|cos| and the tracer multiplies by |cos| once more (tracer.rs:1418, :1441,
    :1461-1471; openpbr.rs:1128-1132, :1155). Every pixel is therefore  integral f(v,l) cos^2(theta_l) L(l) domega.
  * the diffuse slab is scaled by 1 - f_avg_diel (openpbr.rs:442-445) and f_avg_diel is f0_from_ior(specular_ior)
    (openpbr.rs:645, brdf.rs:28-31): Schlick's F0, NOT the hemispherical average of the Fresnel reflectance
    (fresnel_average_mp below: 0.0918 at ior 1.5 where F0 is 0.04).

A third one was found with these tests ("Radiometry"): specular_weight scales only Schlick's F0
(openpbr.rs:488, :503; brdf.rs:10-12), so at specular_weight 0 the dielectric specular lobe still reflects
(1 - v.h)^5 * D * G2 / (4 n.v n.l). The "Lambert" slab of these tests is Lambert plus that residual lobe, and its
albedo depends on the view direction and on specular_roughness. slab_f() states both terms; the residual is what makes
the emissive-sphere series below a recursion over the view cosine instead of a geometric sum.

Local frame throughout: z is the shading normal, v points from the hit to the viewer, l to the light."""
import numpy as np
from scipy import integrate

PI = np.pi
QUAD_TOL = 1e-10


# ---------------------------------------------------------------- Fresnel ----------------------------------------------------------------
def f0_from_ior(ior):  # brdf.rs:28-31
    r = (ior - 1.0) / (ior + 1.0)
    return r * r


def f_avg_diel(ior):  # openpbr.rs:645: the "average" the diffuse slab is scaled by is F0
    return f0_from_ior(ior)


def fresnel_average_mp(ior):
    """Hemispherical (cosine-weighted) average of the exact unpolarised dielectric Fresnel reflectance, by mpmath
    quadrature: 2 * integral_0^1 F(mu) mu dmu. What `1 - F_dielectric_avg` would be by its name."""
    import mpmath as mp
    n = mp.mpf(ior)

    def fresnel(mu):
        st2 = (1 - mu * mu) / (n * n)
        ct = mp.sqrt(1 - st2)
        rs = (mu - n * ct) / (mu + n * ct)
        rp = (n * mu - ct) / (n * mu + ct)
        return (rs * rs + rp * rp) / 2

    return float(2 * mp.quad(lambda mu: fresnel(mu) * mu, [0, 1]))


# ---------------------------------------------------------------- the slab ----------------------------------------------------------------
def alpha_from_roughness(roughness):  # brdf.rs:39-45 at anisotropy 0
    return max(roughness * roughness, 1e-4)


def _ggx_d(h, a):  # brdf.rs:49-54, ax == ay
    t = (h[..., 0] ** 2 + h[..., 1] ** 2) / (a * a) + h[..., 2] ** 2
    return 1.0 / (PI * a * a * t * t)


def _ggx_lambda(w, a):  # brdf.rs:57-63
    return (-1.0 + np.sqrt(1.0 + a * a * (w[..., 0] ** 2 + w[..., 1] ** 2) / np.maximum(w[..., 2] ** 2, 1e-300))) * 0.5


def slab_f(v, l, rho, ior, roughness, specular_weight=0.0):
    """BRDF (no cosine) of the OpenPBR slab these tests use: base_weight 1, base_diffuse_roughness 0 (EON at roughness
    0 is Lambert, brdf.rs:182-209), grey base_color rho, white specular_color, no coat / fuzz / transmission / metal.
    diffuse  (1 - F0) rho / pi                                           openpbr.rs:410-446
    specular F(v.h) D(h) G2(v,l) / (4 n.v n.l), F = Schlick(F0 * specular_weight)   openpbr.rs:448-551
    v, l: [..., 3] unit vectors of the hit frame. Zero below the horizon on either side (openpbr.rs:629-640)."""
    v, l = np.asarray(v, np.float64), np.asarray(l, np.float64)
    v, l = np.broadcast_arrays(v, l)
    up = (v[..., 2] > 0) & (l[..., 2] > 0)
    nv, nl = np.where(up, v[..., 2], 1.0), np.where(up, l[..., 2], 1.0)
    f0 = f0_from_ior(ior)
    a = alpha_from_roughness(roughness)
    h = v + l
    hn = np.linalg.norm(h, axis=-1, keepdims=True)
    h = h / np.where(hn > 0, hn, 1.0)
    vh = np.clip(np.sum(v * h, axis=-1), 0.0, 1.0)
    fres = f0 * specular_weight + (1.0 - f0 * specular_weight) * (1.0 - vh) ** 5
    g2 = 1.0 / (1.0 + _ggx_lambda(v, a) + _ggx_lambda(l, a))
    spec = fres * _ggx_d(h, a) * g2 / (4.0 * nv * nl)
    return np.where(up, (1.0 - f0) * rho / PI + spec, 0.0)


def view_vector(mu_v):
    return np.array([np.sqrt(max(1.0 - mu_v * mu_v, 0.0)), 0.0, mu_v])


# The specular lobe is integrated over the half vector, not over l: with tan^2(theta_h) = alpha^2 u / (1 - u) the measure
# D(h) h.z domega_h is du dphi / (2 pi), and domega_l = 4 (v.h) domega_h, so
#   integral f_spec cos^2 g(n.l) domega_l = integral F G2 (n.l) (v.h) / ((n.v) h.z) g(n.l) du dphi / (2 pi)
# which stays smooth at roughness 0.05 where the lobe is 0.0025 wide. u = 1 - s^2 removes the 1 / h.z end point.
_S_PANELS, _S_ORDER, _N_PHI = 16, 8, 256


def _specular_nodes(mu_v, ior, roughness, specular_weight):
    """-> (n.l, weight) of a quadrature rule R with  sum weight * g(n.l) = integral f_spec(v,l) cos^2(theta_l) g domega_l."""
    a = alpha_from_roughness(roughness)
    x, w = np.polynomial.legendre.leggauss(_S_ORDER)
    edges = np.linspace(0.0, 1.0, _S_PANELS + 1)
    s = np.concatenate([(e1 - e0) / 2 * x + (e1 + e0) / 2 for e0, e1 in zip(edges[:-1], edges[1:])])
    ws = np.concatenate([(e1 - e0) / 2 * w for e0, e1 in zip(edges[:-1], edges[1:])])
    phi = (np.arange(_N_PHI) + 0.5) * (PI / _N_PHI)  # midpoint rule on [0, pi], mirrored
    wphi = 2.0 * PI / _N_PHI
    S, P = np.meshgrid(s, phi, indexing="ij")
    den = np.sqrt(S * S + a * a * (1.0 - S * S))
    hz = S / den                                 # cos(theta_h)
    hs = a * np.sqrt(1.0 - S * S) / den          # sin(theta_h)
    h = np.stack([hs * np.cos(P), hs * np.sin(P), hz], axis=-1)
    mu_v = max(mu_v, 1e-6)
    v = view_vector(mu_v)
    vh = h @ v
    l = 2.0 * vh[..., None] * h - v
    ok = (vh > 0) & (l[..., 2] > 0)
    nl = np.where(ok, l[..., 2], 0.5)
    lsafe = np.where(ok[..., None], l, np.array([0.0, 0.0, 1.0]))
    f0 = f0_from_ior(ior) * specular_weight
    fres = f0 + (1.0 - f0) * (1.0 - np.clip(vh, 0, 1)) ** 5
    g2 = 1.0 / (1.0 + _ggx_lambda(v, a) + _ggx_lambda(lsafe, a))
    # du / h.z = 2 s ds * den / s = 2 den ds
    val = fres * g2 * nl * vh / mu_v * 2.0 * den / (2.0 * PI)
    wt = np.where(ok, val, 0.0) * ws[:, None] * wphi
    return nl.ravel(), wt.ravel()


def albedo(mu_v, rho, ior, roughness, specular_weight=0.0):
    """integral f(v,l) cos^2(theta_l) domega over the hemisphere: what one bounce keeps under the reference's estimator.
    Diffuse part in closed form ((1 - F0) rho * 2/3), specular part by the half-vector quadrature."""
    _, wt = _specular_nodes(mu_v, ior, roughness, specular_weight)
    return (1.0 - f0_from_ior(ior)) * rho * (2.0 / 3.0) + wt.sum()


def albedo_bruteforce(mu_v, rho, ior, roughness, specular_weight=0.0):
    """The same integral by scipy's adaptive quadrature over (cos theta_l, phi): slow, and only reliable for a wide lobe.
    It exists to check the half-vector rule above."""
    v = view_vector(mu_v)

    def g(phi, c):
        s = np.sqrt(1.0 - c * c)
        return float(slab_f(v, np.array([s * np.cos(phi), s * np.sin(phi), c]), rho, ior, roughness, specular_weight)) * c * c

    val, _ = integrate.dblquad(g, 0.0, 1.0, 0.0, PI, epsabs=QUAD_TOL, epsrel=QUAD_TOL)
    return 2.0 * val


# ---------------------------------------------------------------- closed forms ----------------------------------------------------------------
def dome_over_convex(mu_v, radiance, rho, ior, roughness, specular_weight=0.0):
    """A convex body under a uniform dome of the given radiance: every bounce ray escapes, so a pixel is the one-bounce
    integral, radiance * albedo(view), whatever max_depth >= 1 is."""
    return radiance * albedo(mu_v, rho, ior, roughness, specular_weight)


def distant_zero_angle(v, to_light, irradiance, rho, ior, roughness, specular_weight=0.0):
    """A distant light of vanishing angle delivering `irradiance` on a surface facing it (light.rs:255-303: radiance =
    irradiance / Omega inside the cone): f(v,l) cos^2(theta_l) * irradiance."""
    to_light = np.asarray(to_light, np.float64)
    return float(slab_f(v, to_light, rho, ior, roughness, specular_weight)) * to_light[2] ** 2 * irradiance


def emissive_sphere_series(depth, emission, a):
    """Camera inside a closed emissive shell whose every bounce keeps the constant fraction a: Le (1 - a^(d+1)) / (1 - a)."""
    return emission * (1.0 - a ** (depth + 1)) / (1.0 - a)


_INTERIOR_CACHE = {}


def _interior_operator(rho, ior, roughness, specular_weight, n_mu=129):
    """The bounce operator inside a sphere on a grid of cosines. Inside a sphere a ray leaves a vertex at the cosine at
    which it arrives at the next one, so the radiance is a function L(mu) of the arrival cosine alone, and
    (T L)(mu_v) = integral f(v,l) mu_l^2 L(mu_l) domega_l. Diffuse row: 2 (1-F0) rho * Simpson weights * mu^2; specular
    row: the half-vector rule deposited on the grid with linear interpolation."""
    key = (rho, ior, roughness, specular_weight, n_mu)
    if key not in _INTERIOR_CACHE:
        mu = np.linspace(0.0, 1.0, n_mu)
        simpson = np.ones(n_mu)
        simpson[1:-1:2], simpson[2:-1:2] = 4.0, 2.0
        simpson *= (1.0 / (n_mu - 1)) / 3.0
        T = np.tile(2.0 * (1.0 - f0_from_ior(ior)) * rho * simpson * mu * mu, (n_mu, 1))
        for i, m in enumerate(mu):
            nl, wt = _specular_nodes(m, ior, roughness, specular_weight)
            x = nl * (n_mu - 1)
            j = np.minimum(x.astype(np.int64), n_mu - 2)
            t = x - j
            T[i] += np.bincount(j, wt * (1.0 - t), n_mu) + np.bincount(j + 1, wt * t, n_mu)
        _INTERIOR_CACHE[key] = (mu, T)
    return _INTERIOR_CACHE[key]


def emissive_sphere_interior(depth, emission, mu_cam, rho, ior, roughness, specular_weight=0.0):
    """Camera inside an emissive, scattering sphere, no lights, max_depth = depth: L_0 = Le, L_(k+1) = Le + T L_k, the
    pixel is L_depth at the cosine mu_cam under which the camera ray meets the wall (1 from the centre). Without the
    residual specular lobe this is emissive_sphere_series(depth, Le, (1 - F0) rho 2/3)."""
    mu, T = _interior_operator(rho, ior, roughness, specular_weight)
    L = np.full(mu.shape, float(emission))
    for _ in range(depth):
        L = emission + T @ L
    return np.interp(mu_cam, mu, L)


# ---------------------------------------------------------------- quadratures over lights ----------------------------------------------------------------
def _pixel_integrand(v, rho, ior, roughness, specular_weight):
    return lambda l: float(slab_f(v, l, rho, ior, roughness, specular_weight)) * l[2] ** 2


def cone_integral(fn, axis, cos_half):
    """integral of fn(l) domega over the directions of the hit frame within acos(cos_half) of `axis` AND above the horizon.
    A cone wholly above the horizon is integrated in polar coordinates about its axis. One the horizon cuts is integrated
    over (mu = l.z, azimuth) with the cone as the limits of the azimuth,
    |phi - phi_axis| <= acos((cos_half - mu a_z) / (sqrt(1 - mu^2) a_r)), so that fn is smooth inside the limits."""
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    az, ar, phi_a = axis[2], np.hypot(axis[0], axis[1]), np.arctan2(axis[1], axis[0])
    theta_a, beta = np.arccos(np.clip(az, -1.0, 1.0)), np.arccos(cos_half)
    mu_lo = max(0.0, np.cos(min(theta_a + beta, PI)))
    mu_hi = 1.0 if theta_a <= beta else np.cos(theta_a - beta)
    if mu_hi <= mu_lo:
        return 0.0
    if theta_a + beta < PI / 2:
        e1 = np.cross(axis, [0.0, 0.0, 1.0] if abs(az) < 0.9 else [1.0, 0.0, 0.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(axis, e1)

        def about_axis(phi, c):
            return fn(c * axis + np.sqrt(max(1.0 - c * c, 0.0)) * (np.cos(phi) * e1 + np.sin(phi) * e2))

        return integrate.dblquad(about_axis, cos_half, 1.0, 0.0, 2.0 * PI, epsabs=QUAD_TOL, epsrel=QUAD_TOL)[0]

    def half_width(mu):
        s = np.sqrt(max(1.0 - mu * mu, 0.0)) * ar
        if s <= 0.0:
            return PI if mu * az >= cos_half else 0.0
        return float(np.arccos(np.clip((cos_half - mu * az) / s, -1.0, 1.0)))

    def g(dphi, mu):
        s = np.sqrt(max(1.0 - mu * mu, 0.0))
        return fn(np.array([s * np.cos(phi_a + dphi), s * np.sin(phi_a + dphi), mu]))

    # where the cone holds the pole, the azimuth runs the full circle above cos(beta - theta_a): a kink of the limits
    cuts = [mu_lo, mu_hi]
    if theta_a < beta and mu_lo < np.cos(beta - theta_a) < 1.0:
        cuts.insert(1, np.cos(beta - theta_a))
    return sum(integrate.dblquad(g, a, b, lambda mu: -half_width(mu), half_width, epsabs=QUAD_TOL, epsrel=QUAD_TOL)[0]
               for a, b in zip(cuts[:-1], cuts[1:]))


def rect_integral(fn, origin, edge_u, edge_v, normal):
    """integral of fn(l) domega over the directions under which the origin of the hit frame sees the front of the
    one-sided rectangle origin + s edge_u + t edge_v (light.rs:60-80, :180-187), as the integral over its area of
    fn(l) cos_light / d^2."""
    o, eu, ev, n = (np.asarray(a, np.float64) for a in (origin, edge_u, edge_v, normal))
    area = np.linalg.norm(np.cross(eu, ev))

    def g(t, s):
        p = o + s * eu + t * ev
        d2 = p @ p
        l = p / np.sqrt(d2)
        return fn(l) * max(-(n @ l), 0.0) / d2

    return area * integrate.dblquad(g, 0.0, 1.0, 0.0, 1.0, epsabs=QUAD_TOL, epsrel=QUAD_TOL)[0]


def distant_cone(v, to_light, half_angle, irradiance, rho, ior, roughness, specular_weight=0.0):
    """A distant light whose directions fill a cone of the given half angle (radians) around to_light, of radiance
    irradiance / Omega with Omega = 2 pi (1 - cos half_angle) (light.rs:255-303)."""
    ch = np.cos(half_angle)
    return irradiance / (2.0 * PI * (1.0 - ch)) * cone_integral(_pixel_integrand(v, rho, ior, roughness, specular_weight), to_light, ch)


def sphere_cap_solid_angle(distance, radius):
    return 2.0 * PI * (1.0 - np.sqrt(1.0 - (radius / distance) ** 2))


def sphere_light(v, center, radius, radiance, rho, ior, roughness, specular_weight=0.0):
    """A sphere light seen from the origin of the hit frame: its visible cap is the cone of half angle asin(r / d) around
    the centre's direction, less what lies below the horizon."""
    center = np.asarray(center, np.float64)
    d = np.linalg.norm(center)
    return radiance * cone_integral(_pixel_integrand(v, rho, ior, roughness, specular_weight), center / d,
                                    np.sqrt(1.0 - (radius / d) ** 2))


def rect_light(v, origin, edge_u, edge_v, normal, radiance, rho, ior, roughness, specular_weight=0.0):
    """A RectLight facing the plane, seen from the origin of the hit frame."""
    above = _pixel_integrand(v, rho, ior, roughness, specular_weight)
    return radiance * rect_integral(lambda l: above(l) if l[2] > 0.0 else 0.0, origin, edge_u, edge_v, normal)


def _triangle_solid_angle(a, b, c):  # Van Oosterom & Strackee 1983
    la, lb, lc = np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(c)
    num = a @ np.cross(b, c)
    den = la * lb * lc + (a @ b) * lc + (a @ c) * lb + (b @ c) * la
    return 2.0 * np.arctan2(abs(num), den)


def rect_solid_angle(point, origin, edge_u, edge_v):
    """Solid angle a rectangle subtends at a point (0 for a point in its plane)."""
    p, o, eu, ev = (np.asarray(a, np.float64) for a in (point, origin, edge_u, edge_v))
    c0, c1, c2, c3 = o - p, o + eu - p, o + eu + ev - p, o + ev - p
    return _triangle_solid_angle(c0, c1, c2) + _triangle_solid_angle(c0, c2, c3)
