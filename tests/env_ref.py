"""The truth for environment-mapped dome lights (test infrastructure): the reference's EnvironmentMap
(environment.rs:39-214) and the mapped arm of DomeLight (light.rs:320-389) restated in numpy, one float32 operation per
reference operation, as tests/curve_ref.py restates the curve primitives. The oracle knows no mapped dome, so this is
what the host build, the host-compiled device source and the kernels are compared with, bit for bit.

  EnvRef     float32, vectorised. Its sin / cos / acos / atan2 are the DEVICE SOURCE compiled for the host
             (tests/host_shade/env_host.cpp: dmath.hip.h) — the one documented departure from Rust's libm —
             everything else is numpy float32 arithmetic written independently of envmap.hip.h: the bin comes from
             np.searchsorted, the float -> index cast from clip + astype, rem_euclid from np.fmod.
  EnvRef64   float64 with numpy's libm: the analytic checks (energy, normalisation) and their standard errors.

No vendor atan2f / sinf is on the float32 path."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crust-render_amd", "csrc")
HOST_SHADE = os.path.join(ROOT, "tests", "host_shade")
HOST_FLAGS = ["-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes"]

f32, f64, u32 = np.float32, np.float64, np.uint32
PI, TAU = f32(np.pi), f32(2.0 * np.pi)
_F = lambda a: np.ascontiguousarray(a, dtype=f32)


# ---- the device source as host C++ ---------------------------------------------------------------------------------
class Host:
    def __init__(self, out_dir):
        out = os.path.join(str(out_dir), "libenv_host.so")
        cmd = ["g++"] + HOST_FLAGS + ["-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + os.path.join(CSRC, "kernels"),
                                      os.path.join(HOST_SHADE, "env_host.cpp"), "-o", out]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        self.lib = C.CDLL(out)

    def _call(self, name, *args):
        fn = getattr(self.lib, name)
        fn.restype = None
        fn(*[C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a for a in args])

    def atan2(self, y, x):
        y, x = np.broadcast_arrays(_F(y), _F(x))
        y, x = _F(y).reshape(-1), _F(x).reshape(-1)
        o = np.empty_like(y)
        self._call("host_env_atan2_n", y, x, C.c_size_t(y.size), o)
        return o

    def acos(self, x):
        x = _F(x).reshape(-1)
        o = np.empty_like(x)
        self._call("host_env_acos_n", x, C.c_size_t(x.size), o)
        return o

    def sincos(self, x):
        x = _F(x).reshape(-1)
        s, c = np.empty_like(x), np.empty_like(x)
        self._call("host_env_sincos_n", x, C.c_size_t(x.size), s, c)
        return s, c

    def direction_to_uv(self, d):
        d = _F(d).reshape(-1, 3)
        o = np.empty((len(d), 2), f32)
        self._call("host_env_direction_to_uv_n", d, C.c_size_t(len(d)), o)
        return o[:, 0], o[:, 1]

    def uv_to_direction(self, u, v):
        uv = _F(np.stack([_F(u).reshape(-1), _F(v).reshape(-1)], axis=1))
        o = np.empty((len(uv), 3), f32)
        self._call("host_env_uv_to_direction_n", uv, C.c_size_t(len(uv)), o)
        return o

    def bin(self, cdf, steps, u):
        cdf, u = _F(cdf), _F(u).reshape(-1)
        o = np.empty(len(u), u32)
        self._call("host_env_bin_n", cdf, C.c_uint32(len(cdf) - 1), C.c_uint32(steps), u, C.c_size_t(len(u)), o)
        return o

    def sample(self, image, tint, u, v):
        """-> direction [n, 3], radiance [n, 3], pdf [n], some [n] bool (zeros where None)"""
        u, v, tint = _F(u).reshape(-1), _F(v).reshape(-1), _F(tint)
        o = np.empty((len(u), 8), f32)
        self._call("host_env_sample_n", image, tint, u, v, C.c_size_t(len(u)), o)
        return o[:, 0:3].copy(), o[:, 3:6].copy(), o[:, 6].copy(), o[:, 7] != 0

    def escaped(self, image, tint, d):
        d, tint = _F(d).reshape(-1, 3), _F(tint)
        o = np.empty((len(d), 4), f32)
        self._call("host_env_escaped_n", image, tint, d, C.c_size_t(len(d)), o)
        return o[:, 0:3].copy(), o[:, 3].copy()


_HOSTS = {}


def host(out_dir):
    """One build per directory (a module-scoped tmp dir in the tests)."""
    key = str(out_dir)
    if key not in _HOSTS:
        _HOSTS[key] = Host(out_dir)
    return _HOSTS[key]


# ---- float32 restatement ---------------------------------------------------------------------------------------------
def distribution1d(func):
    """Distribution1D::new (environment.rs:40-66) -> (cdf [n + 1] f32, integral f32)."""
    func = _F(func)
    n = len(func)
    running = np.cumsum(func.astype(f64) / f64(n))  # a sequential f64 sum, term by term
    cdf = np.concatenate([[f32(0)], running.astype(f32)]).astype(f32)
    integral = f32(running[-1])
    if integral > 0:
        cdf = (cdf / integral).astype(f32)
    else:
        cdf = (np.arange(n + 1, dtype=f32) / f32(n)).astype(f32)
    return cdf, integral


def _cross(a, b):
    return np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]], dtype=f32)


def _dot(a, b):
    return f32(f32(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def mat3_inverse(m):
    """glam Mat3A::inverse on a 3x3 whose COLUMNS are the axes: cross products, det = z . (x cross y), 1 / det, transpose."""
    m = _F(m).reshape(3, 3)
    x, y, z = m[:, 0].copy(), m[:, 1].copy(), m[:, 2].copy()
    t0, t1, t2 = _cross(y, z), _cross(z, x), _cross(x, y)
    inv = f32(1.0) / _dot(z, t2)
    cols = [(t * inv).astype(f32) for t in (t0, t1, t2)]
    return np.stack(cols, axis=1).T.astype(f32).copy()  # from_cols(...).transpose()


def _mul(m, v):
    """glam Mat3A * Vec3A per row of v: (x * v.x + y * v.y) + z * v.z"""
    m, v = _F(m), _F(v).reshape(-1, 3)
    r = m[:, 0][None, :] * v[:, 0:1]
    r = (r + m[:, 1][None, :] * v[:, 1:2]).astype(f32)
    return (r + m[:, 2][None, :] * v[:, 2:3]).astype(f32)


def _normalize(a):
    d = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).astype(f32) + a[:, 2] * a[:, 2]).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (a / np.sqrt(d)[:, None]).astype(f32)


def _index(f, n):
    """Rust's `(f as usize).min(n - 1)`: the cast saturates, NaN -> 0."""
    g = np.clip(np.nan_to_num(_F(f).astype(f64), nan=0.0, posinf=2.0 ** 40, neginf=0.0), 0.0, 2.0 ** 40)
    return np.minimum(g.astype(np.int64), n - 1)


def _bin(cdf, u):
    """min(the largest i with cdf[i] <= u, n - 1); NaN takes the last bin (the reference's comparator: Less)."""
    n = len(cdf) - 1
    return np.clip(np.searchsorted(cdf, u, side="right").astype(np.int64) - 1, 0, n - 1)


class EnvRef:
    def __init__(self, host_lib, width, height, rgb, light_to_world=None):
        self.m, self.w, self.h = host_lib, int(width), int(height)
        w, h = self.w, self.h
        self.rgb = _F(rgb).reshape(h, w, 3)
        self.l2w = np.eye(3, dtype=f32) if light_to_world is None else _F(light_to_world).reshape(3, 3)
        self.w2l = mat3_inverse(self.l2w)
        theta = ((np.arange(h, dtype=f32) + f32(0.5)) / f32(h) * PI).astype(f32)
        sin_theta = self.m.sincos(theta)[0]
        c = self.rgb
        lum = ((f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]).astype(f32) + f32(0.0722) * c[..., 2]).astype(f32)
        self.cond_func = (np.where(lum > 0, lum, f32(0)).astype(f32) * sin_theta[:, None]).astype(f32)
        rows = [distribution1d(self.cond_func[y]) for y in range(h)]
        self.cond_cdf = np.stack([r[0] for r in rows]).astype(f32)
        self.cond_integral = np.array([r[1] for r in rows], dtype=f32)
        self.marg_func = self.cond_integral.copy()
        self.marg_cdf, self.marg_integral = distribution1d(self.marg_func)

    # environment.rs:156-168
    def direction_to_uv(self, d):
        d = _F(d).reshape(-1, 3)
        with np.errstate(invalid="ignore"):
            y = np.where(d[:, 1] < -1, f32(-1), np.where(d[:, 1] > 1, f32(1), d[:, 1])).astype(f32)
            v = (self.m.acos(y) / PI).astype(f32)
            u = (f32(0.5) + (self.m.atan2(d[:, 0], -d[:, 2]) / TAU).astype(f32)).astype(f32)
            r = np.fmod(u, f32(1.0)).astype(f32)
            u = np.where(r < 0, (r + f32(1.0)).astype(f32), r).astype(f32)
            v = np.where(v < 0, f32(0), np.where(v > 1, f32(1), v)).astype(f32)
        return u, v

    def uv_to_direction(self, u, v):
        u, v = _F(u).reshape(-1), _F(v).reshape(-1)
        st, ct = self.m.sincos((v * PI).astype(f32))
        sp, cp = self.m.sincos(((u - f32(0.5)).astype(f32) * TAU).astype(f32))
        return np.stack([(st * sp).astype(f32), ct, (-(st * cp)).astype(f32)], axis=1).astype(f32)

    def _solid_angle_pdf(self, pdf_uv, v):
        st = self.m.sincos((v * PI).astype(f32))[0]
        k = f32(f32(f32(2.0) * PI) * PI)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            return np.where(st <= 0, f32(0), (pdf_uv / (k * st).astype(f32)).astype(f32)).astype(f32)

    @staticmethod
    def _pdf1(func, integral):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            return np.where(integral > 0, (func / integral).astype(f32), f32(1.0)).astype(f32)

    def lookup(self, local):
        """EnvironmentMap::radiance and ::pdf of local directions -> (texel [n, 3], pdf [n])."""
        u, v = self.direction_to_uv(local)
        with np.errstate(invalid="ignore", over="ignore"):
            x = _index((u * f32(self.w)).astype(f32), self.w)
            y = _index((v * f32(self.h)).astype(f32), self.h)
        texel = self.rgb[y, x]
        if not self.marg_integral > 0:
            return texel, np.zeros(len(u), f32)
        with np.errstate(invalid="ignore", over="ignore"):
            pdf_uv = (self._pdf1(self.cond_func[y, x], self.cond_integral[y]) *
                      self._pdf1(self.marg_func[y], np.full(len(y), self.marg_integral, f32))).astype(f32)
        return texel, self._solid_angle_pdf(pdf_uv, v)

    @staticmethod
    def _sample1(c0, c1, n, u, b):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            span = (c1 - c0).astype(f32)
            within = np.where(span > 0, ((u - c0).astype(f32) / span).astype(f32), f32(0.5)).astype(f32)
            return ((b.astype(f32) + within).astype(f32) / f32(n)).astype(f32)

    def sample(self, u1, u2):
        """EnvironmentMap::sample -> (local direction, texel, pdf, some)."""
        u1, u2 = _F(u1).reshape(-1), _F(u2).reshape(-1)
        n = len(u1)
        if not self.marg_integral > 0:
            return np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros(n, bool)
        row = _bin(self.marg_cdf, u2)
        v = self._sample1(self.marg_cdf[row], self.marg_cdf[row + 1], self.h, u2, row)
        pdf_v = self._pdf1(self.marg_func[row], np.full(n, self.marg_integral, f32))
        col = np.zeros(n, np.int64)
        for y in np.unique(row):
            k = row == y
            col[k] = _bin(self.cond_cdf[y], u1[k])
        u = self._sample1(self.cond_cdf[row, col], self.cond_cdf[row, col + 1], self.w, u1, col)
        pdf_u = self._pdf1(self.cond_func[row, col], self.cond_integral[row])
        d = self.uv_to_direction(u, v)
        with np.errstate(invalid="ignore", over="ignore"):
            pdf = self._solid_angle_pdf((pdf_u * pdf_v).astype(f32), v)
            some = pdf > 0
        texel, _ = self.lookup(d)
        return d, texel, pdf, some

    # light.rs:340-388
    def light_escaped(self, tint, direction):
        """-> radiance [n, 3], pdf [n] (always Some)"""
        texel, pdf = self.lookup(_mul(self.w2l, direction))
        with np.errstate(invalid="ignore", over="ignore"):
            return (_F(tint)[None, :] * texel).astype(f32), pdf

    def light_sample(self, tint, u, v):
        """-> direction [n, 3], radiance [n, 3], pdf [n], some [n]; zeros where None"""
        local, texel, pdf, some = self.sample(u, v)
        with np.errstate(invalid="ignore", over="ignore"):
            d = _normalize(_mul(self.l2w, local))
            rad = (_F(tint)[None, :] * texel).astype(f32)
        z = ~some
        d[z], rad[z], pdf = 0, 0, np.where(some, pdf, f32(0)).astype(f32)
        return d, rad, pdf, some


# ---- float64 restatement (analytic checks) -----------------------------------------------------------------------------
class EnvRef64:
    def __init__(self, width, height, rgb):
        self.w, self.h = int(width), int(height)
        w, h = self.w, self.h
        self.rgb = np.asarray(rgb, dtype=f64).reshape(h, w, 3)
        theta = (np.arange(h) + 0.5) / h * np.pi
        lum = self.rgb @ np.array([0.2126, 0.7152, 0.0722])
        self.func = np.maximum(lum, 0.0) * np.sin(theta)[:, None]
        self.cint = self.func.mean(axis=1)
        self.mint = self.cint.mean()
        with np.errstate(invalid="ignore", divide="ignore"):
            self.ccdf = np.concatenate([np.zeros((h, 1)), np.cumsum(self.func, axis=1) / w / self.cint[:, None]], axis=1)
        for y in np.nonzero(self.cint <= 0)[0]:
            self.ccdf[y] = np.arange(w + 1) / w
        self.mcdf = np.concatenate([[0.0], np.cumsum(self.cint) / h / self.mint]) if self.mint > 0 else np.arange(h + 1) / h

    def exact_mean_rgb_integral(self):
        """The integral of mean(RGB) over the sphere: sum L * (2 pi / w) (cos theta_y - cos theta_{y+1})."""
        edges = np.cos(np.arange(self.h + 1) / self.h * np.pi)
        band = (2.0 * np.pi / self.w) * (edges[:-1] - edges[1:])
        return float((self.rgb.mean(axis=2) * band[:, None]).sum())

    def estimator(self, u1, u2):
        """mean(RGB) / pdf of sample(u1, u2) per draw (0 where None) -> (values, mean, standard error)."""
        u1, u2 = np.asarray(u1, f64), np.asarray(u2, f64)
        h, w = self.h, self.w
        row = np.clip(np.searchsorted(self.mcdf, u2, side="right") - 1, 0, h - 1)
        span = self.mcdf[row + 1] - self.mcdf[row]
        v = (row + np.where(span > 0, (u2 - self.mcdf[row]) / np.where(span > 0, span, 1.0), 0.5)) / h
        col = np.zeros(len(u1), np.int64)
        for y in np.unique(row):
            k = row == y
            col[k] = np.clip(np.searchsorted(self.ccdf[y], u1[k], side="right") - 1, 0, w - 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            pdf_u = np.where(self.cint[row] > 0, self.func[row, col] / self.cint[row], 1.0)
            pdf = pdf_u * (self.cint[row] / self.mint) / (2.0 * np.pi * np.pi * np.sin(v * np.pi))
            x = np.where(pdf > 0, self.rgb[row, col].mean(axis=1) / pdf, 0.0)
        return x, float(x.mean()), float(x.std(ddof=1) / np.sqrt(len(x)))
