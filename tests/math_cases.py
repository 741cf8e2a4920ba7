"""Shared inputs for tests/test_math_host.py and tests/test_gpu_math.py: seeded, nothing read from disk.

unary()      every sign x exponent (2^9) x 2^15 mantissa patterns = 2^24 f32 bit patterns, followed by the edge list.
pow_bulk()   2^24 (x, y) with x drawn per exponent like unary() and y = t / ln x, t uniform in [-87, 88], so every true
             result is a finite normal f32; pow_specials() is the cross product of the special values in both slots.
Test infrastructure."""
import itertools

import numpy as np

F32_MAX = np.float32(3.4028234663852886e38)
PIO2_2_20 = 2.0 ** 20 * (np.pi / 2)  # the sincos accuracy domain: fn * PIO2_HI is exact for fn < 2^20


def _u2f(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def _f2u(f):
    return np.asarray(f, dtype=np.float32).view(np.uint32)


def step(x, k):
    """x moved k f32 steps along the ordered line of floats (through +-0: -0 and +0 are one step apart)."""
    u = _f2u(x).astype(np.int64)
    key = np.where(u & 0x80000000, -(u & 0x7fffffff) - 1, u) + k
    back = np.where(key < 0, ((-key - 1) | 0x80000000), key)
    return _u2f(back.astype(np.uint32))


def mantissas(rows, seed):
    """(rows, 2^15) 23-bit patterns: all-zero, all-one, each single bit set, each single bit clear, then seeded random ones,
    different in every row."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << 23, size=(rows, 1 << 15), dtype=np.uint32)
    one = (np.uint32(1) << np.arange(23, dtype=np.uint32)).astype(np.uint32)
    m[:, 0], m[:, 1] = 0, 0x7fffff
    m[:, 2:25] = one
    m[:, 25:48] = np.uint32(0x7fffff) ^ one
    return m


def grid():
    """2^24 f32: row r = sign * 256 + exponent, 2^15 mantissas each."""
    se = np.arange(512, dtype=np.uint32)[:, None] << np.uint32(23)
    return _u2f((se | mantissas(512, 20240)).reshape(-1))


def edges():
    e = [0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, -1.17549435e-38,
         np.inf, -np.inf, np.nan, 1e5, -1e5, float(F32_MAX), -float(F32_MAX)]
    out = [np.asarray(e, dtype=np.float32)]
    around = [0.5, -0.5, 1.0, -1.0, np.sqrt(2.0), np.sqrt(0.5), 2.0, 1.45e19, -1.45e19, 2.0 ** 62, -2.0 ** 62, 2.0 ** 63,
              709.0, -745.0, 88.72283905206835, -87.33654475055310, -103.97207708399179, 88.73, -103.98,
              np.pi / 4, np.pi / 2, np.pi, 2 * np.pi, 1e7, 1e8]
    a = np.asarray(around, dtype=np.float32)
    out += [step(a, k) for k in (-2, -1, 0, 1, 2)]
    lim = np.float32(PIO2_2_20)
    out += [step(lim, k) for k in range(-4, 5)] + [step(-lim, k) for k in range(-4, 5)]
    return np.concatenate([np.atleast_1d(x) for x in out]).astype(np.float32)


def pio2_multiples(kmax=1 << 21):
    """k * pi/2 rounded to f32 and its two neighbours, k = 1..kmax: the arguments where sin or cos cancels."""
    k = np.arange(1, kmax + 1, dtype=np.float64)
    x = (k * (np.pi / 2)).astype(np.float32)
    return np.concatenate([step(x, -1), x, step(x, 1)])


def unary():
    g = grid()
    return np.concatenate([g, edges(), pio2_multiples(), -pio2_multiples(1 << 12)])


POW_SPECIALS = np.concatenate([
    np.asarray([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, -2.0, 1e-45, 1e-40, -1e-40, 2.0, 0.5, 3.0, -3.0, -0.5],
               dtype=np.float32),
    step(np.float32(1.0), -1).reshape(1), step(np.float32(1.0), 1).reshape(1)])


def pow_bulk(seed=77):
    """(x, y): x = every positive finite exponent x 2^15 mantissas, twice; y = f32(t / ln x), t ~ U[-87, 88]."""
    e = np.arange(255, dtype=np.uint32)[:, None] << np.uint32(23)
    rows = []
    for rep in range(2):
        x = _u2f((e | mantissas(255, 555 + rep)).reshape(-1)).copy()
        x[x == 0] = np.float32(1e-45)
        x[x == 1] = step(np.float32(1.0), 1 - 2 * rep)
        rows.append(x)
    x = np.concatenate(rows)
    pad = (1 << 24) - x.size  # 255 * 2^16 < 2^24: the rest is drawn near 1, where y is large
    rng = np.random.default_rng(seed)
    near1 = (1.0 + rng.uniform(-0.25, 0.25, size=pad)).astype(np.float32)
    k = pad // 2  # half of them log-uniformly close: 1 +- 2^-23 .. 2^-3, exponents up to ~7e8
    near1[:k] = (1.0 + rng.choice([-1.0, 1.0], size=k) * np.exp2(rng.uniform(-23, -3, size=k))).astype(np.float32)
    near1[near1 == 1] = step(np.float32(1.0), 1)
    x = np.concatenate([x, near1])
    t = rng.uniform(-87.0, 88.0, size=x.size)
    y = (t / np.log(x.astype(np.float64))).astype(np.float32)
    return x, y


def pow_specials():
    p = np.asarray(list(itertools.product(POW_SPECIALS, POW_SPECIALS)), dtype=np.float32)
    return p[:, 0].copy(), p[:, 1].copy()


def minmax_cross():
    """NaN / +-0 / ordinary cross product for rmax / rmin / smin / smax, and triples for rclamp."""
    v = np.asarray([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 2.5, float(F32_MAX)], dtype=np.float32)
    neg_nan = _u2f(np.uint32(0xffc00001)).reshape(1)
    v = np.concatenate([v, neg_nan])
    p = np.asarray(list(itertools.product(range(len(v)), repeat=2)))
    t = np.asarray(list(itertools.product(range(len(v)), repeat=3)))
    return (v[p[:, 0]], v[p[:, 1]]), (v[t[:, 0]], v[t[:, 1]], v[t[:, 2]])


def sampler_patterns(drv, n=64):
    """>= 64 sampler patterns: sampler_new of pixel (0, 0) frame 0, other pixels and frames, new_domain chains off them
    and a few raw corner patterns."""
    px = np.asarray([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [255, 255, 0, 0], [256, 0, 0, 0], [3, 5, 1, 0],
                     [17, 200, 7, 0], [0, 0, -1, 0], [1919, 1079, 3, 0], [128, 64, 0, 0], [64, 128, 2, 0], [31, 33, 100, 0],
                     [2, 2, 0x7fffffff, 0], [200, 17, 5, 0]], dtype=np.int32)
    pats = list(drv("sampler_new", px))
    cur = np.asarray(pats, dtype=np.uint32)
    for key in (0, 1, 7, 4096 * 3 + 2, -1):  # tile, bounce, light keys as the integrator chains them
        cur = drv("new_domain", cur, np.full(len(cur), key, dtype=np.int32))
        pats += list(cur)
    pats += [0, 1, 0xffffffff, 0x80000000, 0x9e3779b9]
    pats = np.unique(np.asarray(pats, dtype=np.uint32))
    assert len(pats) >= n
    return pats


def stratified_f32_pairs(n, seed):
    """n pairs of f32 operands stratified over exponent pairs (subnormal operands, and exponents whose sums, products and
    quotients land in the subnormal range or overflow, included), random signs and mantissas."""
    rng = np.random.default_rng(seed)
    ea = (np.arange(n, dtype=np.uint32) % 255)
    eb = ((np.arange(n, dtype=np.uint32) // 255) % 255)
    half = n // 2  # the second half keeps the exponents within 30 of each other, where add / sub round
    eb[half:] = np.clip(ea[half:].astype(np.int64) + rng.integers(-30, 31, size=n - half), 0, 254).astype(np.uint32)

    def make(e):
        s = rng.integers(0, 2, size=n, dtype=np.uint32) << np.uint32(31)
        m = rng.integers(0, 1 << 23, size=n, dtype=np.uint32)
        return _u2f(s | (e << np.uint32(23)) | m)
    return make(ea), make(eb)


def stratified_f64_pairs(n, seed):
    """The same for f64: exponents over all 2047 finite values, subnormals included."""
    rng = np.random.default_rng(seed)
    ea = (np.arange(n, dtype=np.uint64) % 2047)
    eb = ((np.arange(n, dtype=np.uint64) * 7919 // 2047) % 2047)
    half = n // 2
    eb[half:] = np.clip(ea[half:].astype(np.int64) + rng.integers(-60, 61, size=n - half), 0, 2046).astype(np.uint64)

    def make(e):
        s = rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63)
        m = rng.integers(0, 1 << 52, size=n, dtype=np.uint64)
        return (s | (e << np.uint64(52)) | m).view(np.float64)
    return make(ea), make(eb)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a == b
    w = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(w) == b.view(w)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what, *inputs):
    """Bit for bit; a NaN on both sides counts as equal, as everywhere in this suite."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(~same_bits(got, want).reshape(len(got), -1).all(axis=1))
    assert len(bad) == 0, (what, len(bad), [np.asarray(i)[bad[:4]] for i in inputs], got[bad[:4]], want[bad[:4]])


THIN_FILM_THICKNESS = np.asarray([0.5, 1e3, 1e7, 1e18, np.inf], dtype=np.float32)


def thin_film_cases(sc, n=50000):
    """Thin-film materials whose authored thickness runs from ordinary to infinite, and eval queries on them. At 1e18 the
    phase is past the range of the double -> int64 conversion sincos used to make, where x86 and gfx950 answer with
    different quadrants."""
    rng = np.random.default_rng(12)
    mats = sc.materials("thin_film", 250, rng)
    mats["thin_film_thickness"] = np.tile(THIN_FILM_THICKNESS, 50)
    mats["thin_film_weight"] = np.maximum(mats["thin_film_weight"], np.float32(0.5))
    return mats, sc.shade_queries(n, len(mats), rng)


def check_thin_film(sc, mats, q, got, want):
    bad = sc.mismatches(got, want)
    assert len(bad) == 0, (len(bad), got[bad[:2]], want[bad[:2]], mats["thin_film_thickness"][q["material"][bad[:2]]])
    assert np.isfinite(got["value"]).all() and np.isfinite(got["pdf"]).all()
    for t in THIN_FILM_THICKNESS:  # every thickness is evaluated, with light coming back
        sel = mats["thin_film_thickness"][q["material"]] == t
        assert (got["some"][sel] == 1).sum() > 1000 and (got["value"][sel].sum(axis=1) > 0).sum() > 1000, t


# ---- the bare arithmetic against numpy: one correctly rounded IEEE operation per written operation ----------------
def check_f32_arithmetic(dev, n):
    """f32 + - x / sqrt and f32 -> f64 of a driver against numpy on n stratified pairs."""
    a, b = stratified_f32_pairs(n, 5)
    tiny = np.float32(1.17549435e-38)
    with np.errstate(all="ignore"):
        want = {"add_f32": a + b, "sub_f32": a - b, "mul_f32": a * b, "div_f32": a / b}
        for name, w in want.items():
            assert w.dtype == np.float32
            assert_same(dev(name, a, b), w, name, a, b)
            sub = (np.abs(w) < tiny) & (w != 0)
            assert sub.sum() > n >> 14, (name, sub.sum())  # subnormal results are part of the comparison
        assert ((np.abs(a) < tiny) & (a != 0)).sum() > n >> 11 and np.isinf(want["mul_f32"]).any()
        r = np.abs(a)
        assert_same(dev("sqrt_f32", r), np.sqrt(r), "sqrt_f32", r)
        assert_same(dev("sqrt_f32", a), np.sqrt(a), "sqrt_f32 with negative arguments", a)
        assert_same(dev("f32_to_f64", a), a.astype(np.float64), "f32_to_f64", a)


def check_f64_arithmetic(dev, n):
    """f64 + - x / sqrt, f64 -> f32 and rint of a driver against numpy on n stratified pairs."""
    a, b = stratified_f64_pairs(n, 6)
    tiny = 2.2250738585072014e-308
    with np.errstate(all="ignore"):
        want = {"add_f64": a + b, "sub_f64": a - b, "mul_f64": a * b, "div_f64": a / b}
        for name, w in want.items():
            assert_same(dev(name, a, b), w, name, a, b)
            sub = (np.abs(w) < tiny) & (w != 0)
            assert sub.sum() > n >> 14, (name, sub.sum())
        r = np.abs(a)
        assert_same(dev("sqrt_f64", r), np.sqrt(r), "sqrt_f64", r)
        # f64 -> f32: exact products of two f32 (48 significant bits), so most of them round; overflow to inf and
        # subnormal f32 results included
        fa, fb = stratified_f32_pairs(n, 7)
        p = fa.astype(np.float64) * fb.astype(np.float64)
        w = p.astype(np.float32)
        assert_same(dev("f64_to_f32", p), w, "f64_to_f32", p)
        assert ((np.abs(w) < np.float32(1.17549435e-38)) & (w != 0)).sum() > n >> 14 and np.isinf(w).any()
        # rint: ties to even, both signs, magnitudes from below 1/2 up to 2^63
        rng = np.random.default_rng(8)
        k = rng.integers(-2 ** 40, 2 ** 40, size=n >> 2).astype(np.float64)
        t = np.concatenate([k + 0.5, k / 4.0, fa.astype(np.float64)[:n >> 2] * 0.63661977236758138, a[:n >> 2],
                            np.asarray([0.5, -0.5, 1.5, 2.5, -0.0, 0.49999999999999994, 2.0 ** 52 + 1, 2.0 ** 63, np.inf, np.nan])])
        assert_same(dev("rint_f64", t), np.rint(t), "rint_f64", t)


def check_dot_and_normalize(dev, n):
    rng = np.random.default_rng(9)
    a = (rng.standard_normal((n, 3)) * np.exp2(rng.integers(-70, 60, size=(n, 1)))).astype(np.float32)
    b = (rng.standard_normal((n, 3)) * np.exp2(rng.integers(-70, 60, size=(n, 1)))).astype(np.float32)
    with np.errstate(all="ignore"):
        dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]  # one rounding per operation, no contraction
        assert_same(dev("dot", a, b), dot, "dot", a, b)
        nrm = a / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])[:, None]
        assert_same(dev("normalize", a), nrm.astype(np.float32), "normalize", a)
        exact = (a.astype(np.float64) * b.astype(np.float64)).sum(axis=1)
    assert (dot.astype(np.float64) != exact).mean() > 0.5  # a fused multiply-add would be seen
