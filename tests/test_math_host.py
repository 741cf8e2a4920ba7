"""The deterministic math (csrc/kernels/dmath.hip.h = oracle/ora_math.h) and the sampler (qmc.hip.h = ora_qmc.h) against
truth that is not this project's code, without a GPU. Both headers are one author's sequence written twice, so GPU ==
oracle says nothing about a wrong coefficient, branch threshold or table entry: here each function is driven alone
(oracle/ora_mathdrv.c; tests/host_shade/math_host.cpp = the device source as host C++) over tests/math_cases.py and

  a. host-compiled device source == oracle, bit for bit (NaN on both sides equal);
  b. both are < 1 ulp of f32 from float64 libm (error <= 2^-29 f32 ulp), the edge list and the worst / flagged bulk
     cases re-judged with mpmath at 120 bits; the bound is the headers' claim, the measured maxima are in DESIGN.md §2;
  c. sincos is defined for every f32, and its bits for |x| < 2^62 are those of the plain sequence, restated in numpy;
  d. the Sobol directions are Joe-Kuo's by the published recurrence, the byte-sliced table is the XOR it claims, owen is a
     nested scramble, the first 2^m draws are (0, m, 2)-nets and 1-D stratified, pcg_hash matches known answers.

The GPU run of the same cases is tests/test_gpu_math.py."""
import numpy as np
import pytest

import math_cases as mc
import math_drivers as md
from math_cases import assert_same

U = np.uint32
CHUNK = 1 << 22


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return {"oracle": md.oracle(), "host": md.host(tmp_path_factory.mktemp("math_host"))}


@pytest.fixture(scope="module")
def X():
    return mc.unary()


# ---- error in f32 ulps -------------------------------------------------------------------------------------------
def ulp_error(got, truth):
    """|got - truth| / spacing_f32(truth), spacing floored at 2^-149. Overflow: an infinite result stands for 2^128, the
    value round-to-nearest treats it as, and a finite truth beyond 2^128 counts as 2^128, so inf is within an ulp exactly
    where the true value lies past FLT_MAX. NaN where either side is NaN."""
    g = np.asarray(got, dtype=np.float64).copy()
    t = np.asarray(truth, dtype=np.float64)
    t = np.where(np.isfinite(t), np.clip(t, -2.0 ** 128, 2.0 ** 128), t)
    g[np.isposinf(g)], g[np.isneginf(g)] = 2.0 ** 128, -2.0 ** 128
    _, e = np.frexp(np.where(np.isfinite(t), t, 1.0))
    sp = np.ldexp(1.0, np.maximum(e - 1 - 23, -149))
    with np.errstate(invalid="ignore"):
        err = np.abs(g - t) / sp
    return np.where(np.isinf(t), np.where(np.asarray(got, dtype=np.float64) == t, 0.0, np.inf), err)


def mp_error(fn, args, got):
    """The same figure with the truth from mpmath at 120 bits; fn(mp, *mpf args) -> mpf."""
    mp = pytest.importorskip("mpmath")
    out = np.zeros(len(got))
    with mp.workprec(120):
        for i in range(len(got)):
            t = fn(mp, *[mp.mpf(float(a[i])) for a in args])
            t = max(min(t, mp.mpf(2) ** 128), -mp.mpf(2) ** 128)
            g = float(got[i])
            g = mp.mpf(2) ** 128 * (1 if g > 0 else -1) if np.isinf(g) else mp.mpf(g)
            e = mp.frexp(t)[1] if t != 0 else -10 ** 6
            sp = mp.mpf(2) ** max(e - 1 - 23, -149)
            out[i] = float(abs(g - t) / sp)
    return out


FUNCS = {  # name -> (domain mask, float64 libm, mpmath)
    "sin": (lambda x: np.abs(x) <= mc.PIO2_2_20, np.sin, lambda mp, x: mp.sin(x)),
    "cos": (lambda x: np.abs(x) <= mc.PIO2_2_20, np.cos, lambda mp, x: mp.cos(x)),
    "acos": (lambda x: np.abs(x) <= 1, np.arccos, lambda mp, x: mp.acos(x)),
    "exp": (lambda x: (x >= -103.98) & (x <= 88.73), np.exp, lambda mp, x: mp.exp(x)),
    "log": (lambda x: (x > 0) & np.isfinite(x), np.log, lambda mp, x: mp.log(x)),
}


def run_unary(drv, name, x):
    if name == "sin":
        return drv("sincos", x)[0]
    if name == "cos":
        return drv("sincos", x)[1]
    return drv(name, x)


def measure(name, args, got, truth_fn, mp_fn, flag=1.0 - 2.0 ** -20, worst=48):
    """max f32 ulp error over the cases; the `worst` largest and everything at or above `flag` re-judged with mpmath."""
    err = np.concatenate([ulp_error(got[i:i + CHUNK], truth_fn(*[a[i:i + CHUNK].astype(np.float64) for a in args]))
                          for i in range(0, len(got), CHUNK)])
    assert not np.isnan(err).any(), (name, "NaN inside the domain", [a[np.isnan(err)][:4] for a in args])
    order = np.argsort(err)[::-1]
    redo = np.unique(np.concatenate([order[:worst], np.flatnonzero(err >= flag)[:2000]]))
    err[redo] = mp_error(mp_fn, [a[redo] for a in args], got[redo])
    k = int(np.argmax(err))
    return float(err[k]), [float(a[k]) for a in args]


# ---- a. the device source, compiled for the host, is the oracle bit for bit ----------------------------------------
@pytest.mark.parametrize("name", ["sincos", "cos", "acos", "exp", "log"])
def test_unary_functions_of_the_device_source_match_the_oracle(drivers, X, name):
    got, want = drivers["host"](name, X), drivers["oracle"](name, X)
    for g, w in zip(got if name == "sincos" else [got], want if name == "sincos" else [want]):
        assert_same(g, w, name, X)


def test_cos_is_the_cosine_of_sincos(drivers, X):
    for d in drivers.values():
        assert_same(d("cos", X), d("sincos", X)[1], "cos vs sincos", X)


def test_pow_of_the_device_source_matches_the_oracle(drivers):
    for x, y in (mc.pow_bulk(), mc.pow_specials()):
        assert_same(drivers["host"]("pow", x, y), drivers["oracle"]("pow", x, y), "pow", x, y)


def test_min_max_clamp_helpers_match_the_oracle_and_their_stated_rules(drivers):
    (a, b), (x, lo, hi) = mc.minmax_cross()
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        want = {"rmax": np.where((a > b) | nan_b, a, b), "rmin": np.where((a < b) | nan_b, a, b),  # f32::max / min
                "smax": np.where(a > b, a, b), "smin": np.where(a < b, a, b)}  # maxps / minps: second on tie or NaN
        want_clamp = np.where(x < lo, lo, np.where(x > hi, hi, x))
    for d in drivers.values():
        for name, w in want.items():
            assert_same(d(name, a, b), w, name, a, b)
        assert_same(d("rclamp", x, lo, hi), want_clamp, "rclamp", x, lo, hi)
    # what the rules mean where kernels go wrong: NaN and signed zeros
    o = drivers["oracle"]
    one, nan, pz, nz = (np.asarray([v], dtype=np.float32) for v in (1.0, np.nan, 0.0, -0.0))
    assert o("rmax", nan, one)[0] == 1 and o("rmax", one, nan)[0] == 1 and o("rmin", nan, one)[0] == 1  # non-NaN operand
    assert np.isnan(o("smax", one, nan)[0]) and o("smax", nan, one)[0] == 1  # the second operand on NaN
    assert np.signbit(o("rmax", pz, nz)[0]) and not np.signbit(o("rmax", nz, pz)[0])  # second on ties
    assert np.signbit(o("smin", pz, nz)[0]) and np.isnan(o("rclamp", nan, pz, one)[0])
    assert nan_a.any() and nan_b.any()


def test_sampler_functions_of_the_device_source_match_the_oracle(drivers):
    rng = np.random.default_rng(31)
    n = 1 << 20
    a, b = (rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(U) for _ in range(2))
    a[:4], b[:4] = [0, 0xffffffff, 1, 0x80000000], [0, 0xffffffff, 0xffff0000, 1]
    h, o = drivers["host"], drivers["oracle"]
    for name, args in (("pcg_hash", (a,)), ("laine_karras", (a, b)), ("owen", (a, b)), ("unit_f32", (a,)),
                       ("new_domain", (a, b.view(np.int32))), ("draw_rnd1", (a, b)), ("draw_sample4", (a, b)),
                       ("draw_sample4", (a, np.arange(n, dtype=U))),
                       ("sampler_new", (rng.integers(-2 ** 31, 2 ** 31, size=(n, 4)).astype(np.int32),))):
        assert_same(h(name, *args), o(name, *args), name, *args)
    assert np.array_equal(h.table("sobol_dirs"), o.table("sobol_dirs"))
    assert np.array_equal(h.table("sobol_table"), o.table("sobol_table"))


# ---- b. accuracy against libm and mpmath ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FUNCS))
@pytest.mark.parametrize("side", ["oracle", "host"])
def test_unary_accuracy_is_under_one_ulp_on_the_stated_domain(drivers, X, side, name):
    domain, truth, mp_fn = FUNCS[name]
    with np.errstate(invalid="ignore"):
        x = X[domain(X)]
    got = run_unary(drivers[side], name, x)
    worst, at = measure(name, [x], got, truth, mp_fn)
    print("max f32 ulp error of %s (%s) on %d arguments: %.6f at %r" % (name, side, len(x), worst, at))
    assert worst < 1.0, (name, side, worst, at)
    # the edge list in full, with mpmath
    with np.errstate(invalid="ignore"):
        e = mc.edges()
        e = e[domain(e)]
    err = mp_error(mp_fn, [e], run_unary(drivers[side], name, e))
    assert err.max() < 1.0, (name, side, e[np.argmax(err)], err.max())
    if name in ("sin", "cos"):  # 1e5 is the domain the oracle used to state: the least that must hold
        assert (np.abs(x) >= 1e5).sum() > 1 << 20 and np.float32(1e5) in x


@pytest.mark.parametrize("side", ["oracle", "host"])
def test_pow_accuracy_is_under_one_ulp_where_the_result_is_a_finite_normal(drivers, side):
    x, y = mc.pow_bulk()
    got = drivers[side]("pow", x, y)
    truth = np.power(x.astype(np.float64), y.astype(np.float64))
    assert (truth >= 2.0 ** -126).all() and (truth < 2.0 ** 128).all() and len(x) == 1 << 24  # no case is left out
    worst, at = measure("pow", [x, y], got, np.power, lambda mp, a, b: mp.power(a, b))
    print("max f32 ulp error of pow (%s) on %d pairs: %.6f at %r" % (side, len(x), worst, at))
    assert worst < 1.0, (side, worst, at)
    assert (x < 1.17549435e-38).sum() > 1 << 15 and (np.abs(y) > 1e6).sum() > 1000  # subnormal bases, bases next to 1


# ---- branch coverage of the inputs -----------------------------------------------------------------------------------
def test_the_cases_reach_every_branch(X):
    with np.errstate(invalid="ignore", over="ignore"):
        x = X.astype(np.float64)
        dom = np.abs(x) <= mc.PIO2_2_20
        q = np.mod(np.rint(x[dom] * 6.36619772367581382433e-01), 4)
        assert all((q == k).sum() > 10000 for k in range(4))  # the four quadrants of sincos
        assert np.isnan(x).any() and (np.abs(x) >= 2.0 ** 62).any() and ((np.abs(x) > mc.PIO2_2_20) & (np.abs(x) < 2.0 ** 62)).any()
        for sign in (1, -1):  # acos: both arms, both signs, the early returns
            assert ((sign * x > 0) & (np.abs(x) < 0.5)).sum() > 10000 and ((sign * x >= 0.5) & (sign * x < 1)).sum() > 10000
            assert (sign * x >= 1).any() and (x == sign * 0.5).any()
        pos = x[(x > 0) & np.isfinite(x)]
        m = np.frexp(pos)[0] * 2  # [1, 2)
        assert (m > np.sqrt(2.0)).sum() > 10000 and (m <= np.sqrt(2.0)).sum() > 10000  # the sqrt(2) fold of log_d
        assert (x == 0).any() and (x < 0).any() and np.isposinf(x).any()  # log_det's early returns
        assert (x > 709).any() and (x < -745).any()  # exp_d's
        for lo, hi in ((88.0, 88.73), (-103.98, -87.34), (-87.34, -87.0)):  # overflow, subnormal results, just above
            assert ((x > lo) & (x < hi)).sum() > 100
        px, py = mc.pow_specials()
        assert ((py == 0) & np.isnan(px)).any() and (np.isnan(py) & (px == 1)).any() and ((px == 1) & np.isinf(py)).any()
        assert ((px == 0) & (py > 0)).any() and ((px == 0) & (py < 0)).any() and ((px < 0) & (py == -2)).any()
        assert (np.isposinf(px) & (py > 0)).any() and (np.isposinf(px) & (py < 0)).any()
        t = py.astype(np.float64) * np.log(np.where(px > 0, px, 1).astype(np.float64))
        assert (t > 709).any() and (t < -745).any()  # exp_d's early returns through pow


# ---- special values ------------------------------------------------------------------------------------------------
def _f(*v):
    return np.asarray(v, dtype=np.float32)


@pytest.mark.parametrize("side", ["oracle", "host"])
def test_special_values_follow_the_stated_semantics(drivers, side):
    d = drivers[side]
    inf, nan = np.inf, np.nan
    pi32 = np.float32(np.pi)
    ln = d("log", _f(0.0, -0.0, -1.0, -1e-45, -inf, inf, nan, 1.0))
    assert np.isneginf(ln[:2]).all() and np.isnan(ln[2:5]).all() and np.isposinf(ln[5]) and np.isnan(ln[6])  # f32::ln
    assert ln[7] == 0 and not np.signbit(ln[7])
    # acos clamps: f32::acos answers NaN outside [-1, 1]; the one call site passes 1 - 2v for a sample
    # v in [0, 1] (the sphere light's point, light_sample_li), which never leaves [-1, 1]. The current values are asserted so a change is noticed.
    ac = d("acos", _f(1.0, 1.0000001, 2.0, inf, -1.0, -1.0000001, -2.0, -inf, nan, 0.0))
    assert (ac[:4] == 0).all() and (ac[4:8] == pi32).all() and np.isnan(ac[8]) and ac[9] == np.float32(np.pi / 2)
    ex = d("exp", _f(0.0, -0.0, inf, -inf, nan, 88.73, 1000.0, -104.0, -1000.0, 3e38, -3e38))
    assert (ex[:2] == 1).all() and np.isposinf(ex[2]) and ex[3] == 0 and np.isnan(ex[4])
    assert np.isposinf(ex[[5, 6, 9]]).all() and (ex[[7, 8, 10]] == 0).all()  # saturation
    s, c = d("sincos", _f(0.0, -0.0, nan, inf, -inf, 2.0 ** 62, -2.0 ** 62, 3.4e38, 1.45e19))
    # sin(-0) is +0 here (f32::sin keeps the sign): the kernel adds -0 and +0. The value is exact; the path feeds
    # 2 pi u, acos results and thin-film phases, where the sign of a zero sine is multiplied away or squared.
    assert (s[:2] == 0).all() and not np.signbit(s[:2]).any() and (c[:2] == 1).all() and np.isnan(s[2]) and np.isnan(c[2])
    assert (s[3:] == 0).all() and (c[3:] == 1).all()  # the out-of-domain rule: |x| >= 2^62 -> (0, 1)


@pytest.mark.parametrize("side", ["oracle", "host"])
def test_pow_table(drivers, side):
    x, y = mc.pow_specials()
    got = drivers[side]("pow", x, y)
    with np.errstate(all="ignore"):
        ieee = np.power(x.astype(np.float64), y.astype(np.float64))  # C99 pow = f32::powf on the special values
    neg_base = np.signbit(x) & ~np.isnan(x)
    one_nan = (x == 1) & np.isnan(y)
    std = ~neg_base & ~one_nan
    # the standard table: pow(x, 0) = 1 even for NaN, pow(1, y) = 1, NaN otherwise propagates, 0 and inf bases and
    # exponents saturate by sign, everything else within an ulp
    assert_same(np.isnan(got[std]), np.isnan(ieee[std]), "pow NaN table", x[std], y[std])
    fin = std & ~np.isnan(ieee)
    err = ulp_error(got[fin], ieee[fin])
    assert (err < 1.0).all(), (x[fin][err >= 1], y[fin][err >= 1], got[fin][err >= 1])
    exact = fin & (np.isinf(ieee) | (ieee == 0) | (ieee == 1))
    assert np.array_equal(got[exact], ieee[exact].astype(np.float32))
    assert exact.sum() > 60 and ((y == 0) & np.isnan(x) & (got == 1)).any()
    # Departures from f32::powf. The path raises only colours, transmittances and sin^2 in [0, 1] to finite exponents
    # (shade.hip.h: sheen_charlie, coat_passage, sample_transmission_thin), never a negative base or a NaN exponent,
    # so these stay as the headers have them; asserted so that a change is noticed:
    assert np.isnan(got[one_nan]).all() and one_nan.sum() == 1  # powf(1, NaN) = 1; here NaN
    nz = neg_base & (x == 0) & ~np.isnan(y) & (y != 0)  # -0 is treated as +0: powf(-0, -3) = -inf; here +inf
    assert np.array_equal(got[nz], np.where(y[nz] > 0, 0.0, np.inf).astype(np.float32)) and not np.signbit(got[nz]).any()
    neg = neg_base & (x != 0) & ~np.isnan(y) & (y != 0)  # powf(-2, 3) = -8, powf(-2, -2) = 0.25; here NaN
    assert np.isnan(got[neg]).all() and ((x == -2) & (y == 3)).any() and ((x == -2) & (y == -2)).any()
    assert (got[neg_base & (y == 0)] == 1).all() and np.isnan(got[neg_base & np.isnan(y)]).all()


# ---- c. sincos outside its accuracy domain -------------------------------------------------------------------------
_H = float.fromhex
# FreeBSD msun k_sinf.c / k_cosf.c as published (hexadecimal, so no decimal copy of the headers' constants is involved)
MSUN_S = [_H("-0x15555554cbac77.0p-55"), _H("0x111110896efbb2.0p-59"), _H("-0x1a00f9e2cae774.0p-65"), _H("0x16cd878c3b46a7.0p-71")]
MSUN_C = [_H("-0x1ffffffd0c5e81.0p-54"), _H("0x155553e1053a42.0p-57"), _H("-0x16c087e80f1e27.0p-62"), _H("0x199342e0ee5069.0p-68")]
INV_PIO2, PIO2_HI, PIO2_LO = _H("0x1.45f306dc9c883p-1"), _H("0x1.921fb544p+0"), _H("0x1.0b4611a626331p-34")  # e_rem_pio2f.c


def _sincos_plain_sequence(xf):
    """The sequence of dmath.hip.h / ora_math.h restated in numpy float64 (one IEEE operation per ufunc call, no
    contraction), with the quadrant from an int64 conversion — valid for |x| < 2^62 only, like the unguarded code."""
    assert PIO2_HI + PIO2_LO == np.pi / 2 and (PIO2_HI * 2.0 ** 32).is_integer()  # 33 bits: fn * PIO2_HI exact for fn < 2^20
    x = xf.astype(np.float64)
    fn = np.rint(x * INV_PIO2)
    y = (x - fn * PIO2_HI) - fn * PIO2_LO
    n = fn.astype(np.int64) & 3
    z = y * y
    w = z * z
    r = MSUN_S[2] + z * MSUN_S[3]
    s = z * y
    sy = (y + s * (MSUN_S[0] + z * MSUN_S[1])) + s * w * r
    r = MSUN_C[2] + z * MSUN_C[3]
    cy = ((1.0 + z * MSUN_C[0]) + w * MSUN_C[1]) + (w * z) * r
    with np.errstate(over="ignore"):
        sn = np.choose(n, [sy, cy, -sy, -cy]).astype(np.float32)
        cs = np.choose(n, [cy, -sy, -cy, sy]).astype(np.float32)
    return sn, cs


@pytest.mark.parametrize("side", ["oracle", "host"])
def test_sincos_is_defined_for_every_f32_and_unchanged_below_2_to_62(drivers, X, side):
    s, c = drivers[side]("sincos", X)
    with np.errstate(invalid="ignore"):
        ax = np.abs(X.astype(np.float64))
    nan, big = np.isnan(X), ax >= 2.0 ** 62
    assert np.isnan(s[nan]).all() and np.isnan(c[nan]).all()
    assert (s[big] == 0).all() and (c[big] == 1).all() and np.isinf(X[big]).sum() >= 2 and big.sum() > 1 << 20
    rest = ~nan & ~big
    assert np.isfinite(s[rest]).all() and np.isfinite(c[rest]).all()
    for i in range(0, len(X), CHUNK):
        sel = rest[i:i + CHUNK]
        x = X[i:i + CHUNK][sel]
        ws, wc = _sincos_plain_sequence(x)
        assert_same(s[i:i + CHUNK][sel], ws, "sin vs the plain sequence", x)
        assert_same(c[i:i + CHUNK][sel], wc, "cos vs the plain sequence", x)
    assert ((ax > 1.4e19) & rest).sum() == 0 and ((ax > 1e18) & rest).sum() > 1000


def test_thin_film_of_any_authored_thickness_is_finite_and_matches_the_oracle(tmp_path):
    """The reachable input of the conversion defect, through the shading functions (device source as host C++ vs the
    oracle): thin_film_thickness is authored and unclamped and feeds cos_det(2 pi 2 eta thickness cos / lambda). The GPU
    run of this case is in tests/test_gpu_math.py."""
    import ctypes as C
    import os
    import subprocess
    import seam_cases as sc
    out = str(tmp_path / "libseam_host.so")
    cmd = ["g++"] + md.HOST_FLAGS + ["-I" + os.path.join(md.ROOT, "profiles", "host_shade"), "-I" + os.path.join(md.CSRC, "kernels"),
                                     os.path.join(md.HOST_SHADE, "seam_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    mats, q = mc.thin_film_cases(sc)
    got, want = sc.Drivers(C.CDLL(out), "host").eval(mats, q), sc.oracle_drivers().eval(mats, q)
    mc.check_thin_film(sc, mats, q, got, want)


def test_host_build_of_the_primitive_drivers_agrees_with_numpy(drivers):
    """The checks tests/test_gpu_math.py makes of gfx950's arithmetic, on the host build: that g++ without contraction and
    numpy agree is the premise of using numpy as the device's judge."""
    mc.check_f32_arithmetic(drivers["host"], 1 << 20)
    mc.check_f64_arithmetic(drivers["host"], 1 << 20)
    mc.check_dot_and_normalize(drivers["host"], 1 << 18)


# ---- d. the sampler ------------------------------------------------------------------------------------------------
JOE_KUO = [None, (1, 0, (1,)), (2, 1, (1, 3)), (3, 1, (1, 3, 1))]  # new-joe-kuo-6.21201, d = 2, 3, 4: s, a, m_i


def joe_kuo_directions(dim):
    """32 direction numbers, MSB first, by the recurrence of Joe & Kuo 2008 (Bratley & Fox 1988):
    v_i = m_i 2^(32-i) for i <= s; v_i = v_(i-s) ^ (v_(i-s) >> s) ^ XOR_k a_k v_(i-k) for i > s."""
    if JOE_KUO[dim] is None:
        return [1 << (31 - i) for i in range(32)]
    s, a, m = JOE_KUO[dim]
    v = [m[i] << (31 - i) for i in range(s)]
    for i in range(s, 32):
        x = v[i - s] ^ (v[i - s] >> s)
        for k in range(1, s):
            if (a >> (s - 1 - k)) & 1:
                x ^= v[i - k]
        v.append(x)
    return v


@pytest.mark.parametrize("side", ["oracle", "host"])
def test_sobol_directions_are_joe_kuos_and_the_sliced_table_is_their_xor(drivers, side):
    dirs = drivers[side].table("sobol_dirs").reshape(4, 32)
    want = np.asarray([joe_kuo_directions(d) for d in range(4)], dtype=np.uint64).astype(U)
    assert np.array_equal(dirs, want), np.argwhere(dirs != want)
    tab = drivers[side].table("sobol_table").reshape(3, 4, 256)
    for d in range(3):
        for k in range(4):
            for v in range(256):
                x = 0
                for b in range(8):
                    if (v >> b) & 1:
                        x ^= int(want[d + 1][8 * k + b])
                assert int(tab[d, k, v]) == x, (d, k, v)


@pytest.mark.parametrize("side", ["oracle", "host"])
def test_owen_is_a_nested_scramble(drivers, side):
    d = drivers[side]
    rng = np.random.default_rng(8)
    seeds = np.concatenate([np.asarray([0, 1, 0xffffffff, 0x0000ffff, 0xffff0000], dtype=U),
                            rng.integers(0, 1 << 32, size=11, dtype=np.uint64).astype(U)])
    prefix = np.arange(1 << 16, dtype=U)
    for seed in seeds:
        sv = np.full(1 << 16, seed, dtype=U)
        top = d("owen", prefix << U(16), sv) >> U(16)
        low = rng.integers(0, 1 << 16, size=1 << 16, dtype=np.uint64).astype(U)
        assert np.array_equal(d("owen", (prefix << U(16)) | low, sv) >> U(16), top)  # lower bits never reach upward
        for m in range(1, 17):  # the leading m bits are a permutation of the leading m bits, for every m
            out_m, in_m = top >> U(16 - m), prefix >> U(16 - m)
            first = out_m[:: 1 << (16 - m)]
            assert np.array_equal(out_m, first[in_m]) and len(np.unique(first)) == 1 << m, (seed, m)
    # 32 bits, by flips: flipping input bit k flips output bit k and nothing above it
    n = 1 << 18
    x, seed = (rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(U) for _ in range(2))
    base = d("owen", x, seed)
    for k in range(32):
        diff = base ^ d("owen", x ^ U(1 << k), seed)
        assert ((diff >> U(k)) == 1).all(), (k, x[(diff >> U(k)) != 1][:4])
    assert len(np.unique(d("owen", np.arange(1 << 20, dtype=U), np.full(1 << 20, 12345, dtype=U)))) == 1 << 20


@pytest.mark.parametrize("side", ["oracle", "host"])
def test_draws_are_nets_and_stratified(drivers, side):
    d = drivers[side]
    pats = mc.sampler_patterns(d)
    assert len(pats) >= 64 and d("sampler_new", np.zeros((1, 4), dtype=np.int32))[0] in pats
    P, N = len(pats), 1 << 16
    u = d("draw_sample4", np.repeat(pats, N), np.tile(np.arange(N, dtype=U), P)).reshape(P, N, 4)
    assert (u >= 0).all() and (u < 1).all()
    fix = (u.astype(np.float64) * 2.0 ** 24).astype(np.int64)  # unit_f32 keeps 24 bits: exact
    assert np.array_equal(fix / 2.0 ** 24, u)
    for m in range(1, 17):  # every dimension, 1-D: one point per interval of length 2^-m among the first 2^m
        cells = np.sort(fix[:, :1 << m, :] >> (24 - m), axis=1)
        assert (cells == np.arange(1 << m)[None, :, None]).all(), (side, m)
    for m in range(1, 13):  # dimensions (0, 1): one point in every elementary interval of area 2^-m, every split
        for a in range(m + 1):
            b = m - a
            cells = np.sort(((fix[:, :1 << m, 0] >> (24 - a)) << b) | (fix[:, :1 << m, 1] >> (24 - b)), axis=1)
            assert (cells == np.arange(1 << m)[None, :]).all(), (side, m, a)
    r = d("draw_rnd1", np.repeat(pats, 4096), np.tile(np.arange(4096, dtype=U), P))
    assert (r >= 0).all() and (r < 1).all() and abs(r.mean() - 0.5) < 0.005


@pytest.mark.parametrize("side", ["oracle", "host"])
def test_unit_f32_stays_below_one_and_pcg_hash_matches_known_answers(drivers, side):
    d = drivers[side]
    un = d("unit_f32", np.asarray([0xffffffff, 0, 0xffffff00, 0xff, 0x100, 0x80000000], dtype=U))
    assert un[0] == np.float32(1.0 - 2.0 ** -24) and un[0] < 1 and un[1] == 0 and un[2] == un[0] and un[3] == 0
    assert un[4] == np.float32(2.0 ** -24) and un[5] == 0.5

    def pcg_rxs_m_xs(v):  # O'Neill 2014, 32-bit RXS-M-XS output on one LCG step (Jarzynski & Olano 2020), in integers
        state = (v * 747796405 + 2891336453) & 0xffffffff
        word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xffffffff
        return (word >> 22) ^ word
    vals = [0, 1, 0xffffffff, 0x9e3779b9, 12345]
    assert [pcg_rxs_m_xs(v) for v in vals[:3]] == PCG_KNOWN
    assert [int(h) for h in d("pcg_hash", np.asarray(vals, dtype=U))] == [pcg_rxs_m_xs(v) for v in vals]
    # sampler_new / new_domain are the stated compositions of it
    assert int(d("sampler_new", np.asarray([[3, 5, 7, 9]], dtype=np.int32))[0]) == pcg_rxs_m_xs(pcg_rxs_m_xs(7) ^ (3 | (5 << 8)))
    assert int(d("sampler_new", np.asarray([[256 + 3, 512 + 5, 7, 0]], dtype=np.int32))[0]) == pcg_rxs_m_xs(pcg_rxs_m_xs(7) ^ (3 | (5 << 8)))
    assert int(d("new_domain", np.asarray([77], dtype=U), np.asarray([2], dtype=np.int32))[0]) == pcg_rxs_m_xs((77 + 0x9e3779b9 * 3) & 0xffffffff)


# pcg_hash(0), pcg_hash(1), pcg_hash(0xffffffff), worked by hand from the published constants:
#   v = 0:          state = 0xac564b05, shift = 0xa + 4 = 14, word = (state >> 14 ^ state) * 277803737 = 0x07bb2ffc
#   v = 1:          state = 0xd8e8c2ba, shift = 0xd + 4 = 17, word = 0xa8bee89e
#   v = 0xffffffff: state = 0x7fc3d350, shift = 0x7 + 4 = 11, word = 0xe62a4a9a;   result = word >> 22 ^ word
PCG_KNOWN = [0x07bb2fe2, 0xa8beea3c, 0xe62a4902]


# ---- the device driver builds for gfx950 without a GPU -------------------------------------------------------------
def test_device_driver_cross_compiles_for_gfx950_with_the_products_flags(tmp_path):
    flags = md.product_hipflags()
    assert "-fno-slp-vectorize" in flags and "-fno-fast-math" in flags
    so = md.build_device(tmp_path)
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, timeout=60).stdout
    for name in list(md.OPS) + list(md.PRIMITIVES):
        assert "dev_m_%s_n" % name in syms, name
    assert "dev_m_sobol_table" in syms and "dev_m_sobol_dirs" in syms
