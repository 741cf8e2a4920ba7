"""Environment-mapped dome lights without a GPU: atan2_det's accuracy, the environment object the host builds, the device
functions (kernels/envmap.hip.h compiled as host C++, tests/host_shade/env_host.cpp) against the float32 restatement
(tests/env_ref.py), the reference's own unit tests (environment.rs:229-404), the energy the importance sampling must
conserve, the USD importer and the C ABI. The GPU run of the same functions is tests/test_gpu_environment.py.
No vendor atan2f / sinf is on the tested path: the restatement's transcendentals are the device source's."""
import ctypes as C
import os
import pickle
import warnings

import numpy as np
import pytest

import env_cases as ec
import env_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, u32 = np.float32, np.float64, np.uint32


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return er.host(tmp_path_factory.mktemp("env_host"))


@pytest.fixture(scope="module")
def maps(crt):
    return ec.maps(crt)


@pytest.fixture(scope="module")
def built(crt, H, maps):
    """name -> (Environment of the package, its tables, the float32 restatement): each built once, left unchanged."""
    out = {}
    for name, (w, h, rgb, m) in maps.items():
        env = crt.Environment(w, h, rgb, m)
        out[name] = (env, env.tables(), er.EnvRef(H, w, h, rgb, m))
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == bool or b.dtype == bool:
        return np.array_equal(a, b)
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return a.shape == b.shape and bool(np.all((a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))))


# ---- 1. atan2_det ----------------------------------------------------------------------------------------------------
def ulp_error(got, truth):
    """|got - truth| / spacing_f32(truth), spacing floored at 2^-149 (the figure of tests/test_math_host.py)."""
    g, t = np.asarray(got, dtype=f64), np.asarray(truth, dtype=f64)
    _, e = np.frexp(np.where(np.isfinite(t), t, 1.0))
    sp = np.ldexp(1.0, np.maximum(e - 1 - 23, -149))
    with np.errstate(invalid="ignore"):
        return np.abs(g - t) / sp


def mp_ulp_error(y, x, got):
    mp = pytest.importorskip("mpmath")
    out = np.zeros(len(got))
    with mp.workprec(120):
        for i in range(len(got)):
            t = mp.atan2(mp.mpf(float(y[i])), mp.mpf(float(x[i])))
            e = mp.frexp(t)[1] if abs(t) > mp.mpf(2) ** -400 else -10 ** 6
            out[i] = float(abs(mp.mpf(float(got[i])) - t) / mp.mpf(2) ** max(e - 1 - 23, -149))
    return out


PI32 = f32(np.pi)
INF, NAN = f32(np.inf), f32(np.nan)
# (y, x, expected): the special cases dmath.hip.h writes down. +-0 results are compared with their sign.
SPECIAL = [
    (0.0, 1.0, 0.0), (-0.0, 1.0, -0.0), (0.0, -1.0, PI32), (-0.0, -1.0, -PI32),        # the u seam
    (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, -0.0, PI32), (-0.0, -0.0, -PI32),
    (0.0, INF, 0.0), (-0.0, INF, -0.0), (0.0, -INF, PI32), (-0.0, -INF, -PI32),
    (1.0, 0.0, f32(np.pi / 2)), (-1.0, 0.0, -f32(np.pi / 2)), (1.0, -0.0, f32(np.pi / 2)), (-1.0, -0.0, -f32(np.pi / 2)),
    (INF, INF, f32(np.pi / 4)), (-INF, INF, -f32(np.pi / 4)), (INF, -INF, f32(3 * np.pi / 4)), (-INF, -INF, -f32(3 * np.pi / 4)),
    (1.0, INF, 0.0), (-1.0, INF, -0.0), (1.0, -INF, PI32), (-1.0, -INF, -PI32),
    (INF, 1.0, f32(np.pi / 2)), (-INF, -1.0, -f32(np.pi / 2)), (INF, 0.0, f32(np.pi / 2)),
    (1.0, 1.0, f32(np.pi / 4)), (1.0, -1.0, f32(3 * np.pi / 4)), (-1.0, -1.0, -f32(3 * np.pi / 4)),
    (1e-45, 3e38, 0.0), (-1e-45, 3e38, -0.0), (1e-45, -3e38, PI32), (3e38, 1e-45, f32(np.pi / 2)),
    (NAN, 1.0, NAN), (1.0, NAN, NAN), (NAN, NAN, NAN), (NAN, INF, NAN), (0.0, NAN, NAN), (INF, NAN, NAN),
]


def test_atan2_special_cases(H):
    y, x, want = (np.array([c[k] for c in SPECIAL], dtype=f32) for k in range(3))
    got = H.atan2(y, x)
    bad = [(SPECIAL[i], got[i]) for i in range(len(got))
           if not (got[i].view(u32) == want[i].view(u32) or (np.isnan(got[i]) and np.isnan(want[i])))]
    assert not bad, bad
    fin = np.isfinite(y) & np.isfinite(x) & (y != 0) & (x != 0)  # the others are exact, compared by bits above
    assert mp_ulp_error(y[fin], x[fin], got[fin]).max() < 1.0


def test_atan2_within_one_ulp_over_every_sign_and_exponent_pair(H):
    """Every sign x exponent pair of (y, x) (255 exponent fields: subnormals and zero's field included), 2^7 seeded
    mantissa pairs each, against float64 libm (error <= 2^-29 f32 ulp); the 48 worst re-judged with mpmath at 120 bits.
    Bound: < 1 f32 ulp, the contract of dmath.hip.h. The measured maximum is printed (DESIGN.md §2 records it)."""
    rng = np.random.default_rng(2024)
    ex = np.arange(255, dtype=u32)
    worst = []  # (err, y, x, got)
    overall = 0.0
    for ey in range(255):
        my = rng.integers(0, 1 << 23, size=(4, 255, 128), dtype=np.int64).astype(u32)
        mx = rng.integers(0, 1 << 23, size=(4, 255, 128), dtype=np.int64).astype(u32)
        sy = (np.array([0, 0, 1, 1], dtype=u32) << 31)[:, None, None]
        sx = (np.array([0, 1, 0, 1], dtype=u32) << 31)[:, None, None]
        y = (sy | u32(ey << 23) | my).astype(u32).view(f32).reshape(-1)
        x = (sx | (ex[None, :, None] << 23) | mx).astype(u32).view(f32).reshape(-1)
        got = H.atan2(y, x)
        err = ulp_error(got, np.arctan2(y.astype(f64), x.astype(f64)))
        assert not np.isnan(got).any()
        k = np.argsort(err)[-4:]
        worst += [(err[i], y[i], x[i], got[i]) for i in k]
        overall = max(overall, float(err.max()))
    print("atan2_det: max error against float64 libm %.9f f32 ulp over %d pairs" % (overall, 255 * 255 * 4 * 128))
    assert overall < 1.0
    worst = sorted(worst, key=lambda t: t[0])[-48:]
    y, x, got = (np.array([w[k] for w in worst], dtype=f32) for k in (1, 2, 3))
    e = mp_ulp_error(y, x, got)
    print("atan2_det: the 48 worst re-judged with mpmath: max %.9f f32 ulp" % e.max())
    assert e.max() < 1.0


# ---- 2. the reference's own unit tests (environment.rs:229-404) ------------------------------------------------------
class RefSide:
    """The float32 restatement behind the reference's method names (tint 1, identity orientation)."""

    def __init__(self, H, w, h, rgb):
        self.r = er.EnvRef(H, w, h, rgb)
        self.direction_to_uv, self.uv_to_direction = self.r.direction_to_uv, self.r.uv_to_direction

    def sample(self, u1, u2):
        return self.r.light_sample(np.ones(3, f32), u1, u2)

    def pdf(self, d):
        return self.r.lookup(d)[1]


class HostSide:
    """The device source compiled for the host, on the image the package built."""

    def __init__(self, crt, H, w, h, rgb):
        self.H, self.env = H, crt.Environment(w, h, rgb)
        self.image = self.env.tables()["image"]
        self.direction_to_uv, self.uv_to_direction = H.direction_to_uv, H.uv_to_direction

    def sample(self, u1, u2):
        return self.H.sample(self.image, np.ones(3, f32), u1, u2)

    def pdf(self, d):
        return self.H.escaped(self.image, np.ones(3, f32), d)[1]


@pytest.fixture(params=["restatement", "device source on the host"])
def side(request, crt, H):
    if request.param == "restatement":
        return lambda w, h, rgb: RefSide(H, w, h, rgb)
    return lambda w, h, rgb: HostSide(crt, H, w, h, rgb)


def _unit(v):
    v = np.asarray(v, dtype=f64)
    return (v / np.linalg.norm(v)).astype(f32)


def test_ref_direction_and_uv_round_trip(side):
    m = side(1, 1, np.ones((1, 1, 3), f32))
    d = np.array([(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), _unit((0.3, 0.5, -0.8)),
                  _unit((-0.6, -0.2, 0.7))], dtype=f32)
    u, v = m.direction_to_uv(d)
    back = m.uv_to_direction(u, v)
    assert (np.linalg.norm(back.astype(f64) - d, axis=1) < 1e-4).all()


def test_ref_conventions_are_as_documented(side):
    m = side(1, 1, np.ones((1, 1, 3), f32))
    u, v = m.direction_to_uv(np.array([(0, 0, -1), (0, 1, 0), (0, -1, 0)], dtype=f32))
    assert abs(u[0] - 0.5) < 1e-5 and abs(v[0] - 0.5) < 1e-5
    assert v[1] < 1e-5 and v[2] > 1.0 - 1e-5


def test_ref_sample_and_pdf_agree(side):
    m = side(64, 32, ec.spotty(64, 32, 40, 8))
    rng = np.random.default_rng(11)
    d, _rad, pdf, some = m.sample(rng.random(3000, dtype=f32), rng.random(3000, dtype=f32))
    q = m.pdf(d[some])
    assert some.sum() > 2900
    assert (np.abs(pdf[some] - q) <= 1e-3 * np.maximum(pdf[some], q)).all()


def test_ref_pdf_is_normalized_over_the_sphere(side):
    m = side(32, 16, ec.spotty(32, 16, 20, 6))
    rng = np.random.default_rng(5)
    n = 200_000
    _d, _rad, pdf, some = m.sample(rng.random(n, dtype=f32), rng.random(n, dtype=f32))
    estimate = (1.0 / pdf[some & (pdf > 0)].astype(f64)).sum() / n
    assert abs(estimate - 4.0 * np.pi) < 0.05 * 4.0 * np.pi, estimate


def test_ref_sampling_concentrates_on_bright_texels(side):
    w, h, bx, by = 32, 16, 20, 6
    m = side(w, h, ec.spotty(w, h, bx, by))
    rng = np.random.default_rng(3)
    d, _rad, _pdf, some = m.sample(rng.random(20_000, dtype=f32), rng.random(20_000, dtype=f32))
    u, v = m.direction_to_uv(d[some])
    x, y = np.minimum((u * f32(w)).astype(np.int64), w - 1), np.minimum((v * f32(h)).astype(np.int64), h - 1)
    assert ((x == bx) & (y == by)).mean() > 0.5


def test_ref_uniform_map_has_uniform_solid_angle_pdf(side):
    w, h = 32, 16
    m = side(w, h, np.ones((h, w, 3), f32))
    v = ((np.arange(h, dtype=f32) + f32(0.5)) / f32(h)).astype(f32)
    pdf = m.pdf(m.uv_to_direction(np.full(h, f32(0.5) / f32(w), f32), v))
    expected = 1.0 / (4.0 * np.pi)
    assert (np.abs(pdf - expected) < 0.01 * expected).all(), pdf


def test_ref_poles_are_not_oversampled(side):
    w, h = 64, 32
    m = side(w, h, np.ones((h, w, 3), f32))
    v = ((np.array([0, h // 2], dtype=f32) + f32(0.5)) / f32(h)).astype(f32)
    pole, equator = m.pdf(m.uv_to_direction(np.full(2, f32(0.5) / f32(w), f32), v))
    assert abs(pole - equator) < 0.02 * equator


def test_ref_rejects_malformed_buffers(crt):
    with pytest.raises(crt.CrtError, match="1 .. 16384"):
        crt.Environment(0, 4, np.zeros(0, f32))
    with pytest.raises(ValueError):
        crt.Environment(4, 4, np.ones((3, 3), f32))


def test_ref_black_map_declines_to_sample(side):
    m = side(8, 4, np.zeros((4, 8, 3), f32))
    _d, _rad, _pdf, some = m.sample(np.array([0.5], f32), np.array([0.5], f32))
    assert not some.any()
    assert m.pdf(np.array([(0, 1, 0)], dtype=f32))[0] == 0.0


# ---- 3. the tables the host builds == the restatement ----------------------------------------------------------------
def test_tables_equal_the_restatement(built):
    for name, (_env, T, R) in built.items():
        assert (T["width"], T["height"]) == (R.w, R.h), name
        for key, want in (("conditional_func", R.cond_func), ("conditional_cdf", R.cond_cdf),
                          ("conditional_integral", R.cond_integral), ("marginal_func", R.marg_func),
                          ("marginal_cdf", R.marg_cdf), ("light_to_world", R.l2w), ("world_to_light", R.w2l)):
            assert np.array_equal(T[key], want), (name, key)
        assert T["marginal_integral"] == R.marg_integral, name
        assert np.allclose(T["world_to_light"].astype(f64) @ T["light_to_world"].astype(f64), np.eye(3), atol=1e-6), name
    # the paths the hand-made map exists for
    R = built["hand_8x4"][2]
    assert R.cond_integral[2] == 0 and np.array_equal(R.cond_cdf[2], np.arange(9, dtype=f32) / f32(8))  # uniform-row fallback
    assert R.cond_cdf[1][3] == R.cond_cdf[1][4] == R.cond_cdf[1][5] and R.cond_cdf[1][0] == R.cond_cdf[1][1] == 0
    assert R.cond_cdf[1][7] == R.cond_cdf[1][8] == 1 and R.marg_cdf[2] == R.marg_cdf[3]
    assert built["black_8x4"][1]["marginal_integral"] == 0


def test_image_layout(built):
    """One allocation, arrays on 256-byte boundaries: float4 texels (r, g, b, conditional func), float2 rows (conditional
    integral, marginal func), the conditional CDFs, the marginal CDF."""
    for name, (_env, T, R) in built.items():
        im = T["image"]
        hd = im[:40].view(u32)
        w, h = int(hd[0]), int(hd[1])
        assert (w, h) == (R.w, R.h) and im[8:12].view(f32)[0] == R.marg_integral, name
        steps_w, steps_h, off_t, off_r, off_c, off_m, nbytes = (int(x) for x in hd[3:10])
        assert (1 << steps_w) >= w + 1 > (1 << steps_w) >> 1 and (1 << steps_h) >= h + 1 > (1 << steps_h) >> 1, name
        assert all(o % 256 == 0 for o in (off_t, off_r, off_c, off_m, nbytes)) and nbytes == len(im), name
        tex = im[off_t:off_t + w * h * 16].view(f32).reshape(h, w, 4)
        assert np.array_equal(tex[..., :3], R.rgb) and np.array_equal(tex[..., 3], R.cond_func), name
        rows = im[off_r:off_r + h * 8].view(f32).reshape(h, 2)
        assert np.array_equal(rows[:, 0], R.cond_integral) and np.array_equal(rows[:, 1], R.marg_func), name
        assert np.array_equal(im[off_c:off_c + h * (w + 1) * 4].view(f32).reshape(h, w + 1), R.cond_cdf), name
        assert np.array_equal(im[off_m:off_m + (h + 1) * 4].view(f32), R.marg_cdf), name


# ---- 4. the device source on the host == the restatement, bit for bit ------------------------------------------------
def test_bin_rule_takes_the_last_of_equal_entries(H, built):
    """The documented departure: where several CDF entries equal u, the LAST is taken; NaN takes the last bin and a
    negative u the first, as the reference's comparator decides them."""
    R = built["hand_8x4"][2]
    cdf = R.cond_cdf[1]  # 0 0 . . c c c . 1  (bins 0, 3, 4 and 7 have weight 0)
    u = np.array([0.0, cdf[3], 1.0, np.nan, -1.0, f32(1.0) - f32(2.0 ** -24)], dtype=f32)
    got = H.bin(cdf, 4, u)
    assert list(got) == [1, 5, 7, 7, 0, 6], got
    assert np.array_equal(got, er._bin(cdf, u))
    for steps in (4, 5, 9):  # more steps than needed change nothing
        assert np.array_equal(H.bin(cdf, steps, u), got)


def test_device_source_equals_the_restatement(H, built):
    for name, (_env, T, R) in built.items():
        rng = np.random.default_rng(sum(map(ord, name)))
        eu, ev = ec.edge_uv(R)
        u = np.concatenate([rng.random(20_000, dtype=f32), eu])
        v = np.concatenate([rng.random(20_000, dtype=f32), ev])
        got, want = H.sample(T["image"], ec.TINT, u, v), R.light_sample(ec.TINT, u, v)
        for k, what in enumerate(("direction", "radiance", "pdf", "some")):
            assert same_bits(got[k], want[k]), (name, "sample", what)
        if name.startswith("black"):
            assert not got[3].any()
        else:
            assert got[3][:20_000].mean() > 0.99, name
        d = np.concatenate([ec.random_directions(rng, 20_000), ec.edge_directions(R)])
        got, want = H.escaped(T["image"], ec.TINT, d), R.light_escaped(ec.TINT, d)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (name, "escaped")
        gu, gv = H.direction_to_uv(d)
        wu, wv = R.direction_to_uv(d)
        assert same_bits(gu, wu) and same_bits(gv, wv), (name, "direction_to_uv")
        fu, fv = np.isfinite(gu), np.isfinite(gv)
        assert ((gu[fu] >= 0) & (gu[fu] <= 1)).all() and ((gv[fv] >= 0) & (gv[fv] <= 1)).all()


# ---- 5. energy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sky_env", "spotty_64x32", "hand_8x4", "3x2"])
def test_importance_sampling_conserves_energy(H, built, maps, name):
    """mean(radiance / pdf) over 2^16 seeded draws of the host-compiled device functions against the exact float64 texel
    sum, sum L (2 pi / w)(cos theta_y - cos theta_{y+1}) (L = mean of RGB). Margin: 5 standard errors, the error being the
    one the FLOAT64 restatement reports for the same draws — not a figure of the code under test. Negative texels carry
    weight 0 and are never sampled, so the exact sum is taken over the non-negative part of the map."""
    w, h, rgb, _m = maps[name]
    T = built[name][1]
    rng = np.random.default_rng(99)
    u, v = rng.random(1 << 16, dtype=f32), rng.random(1 << 16, dtype=f32)
    lum = rgb.astype(f64) @ np.array([0.2126, 0.7152, 0.0722])
    R64 = er.EnvRef64(w, h, np.where((lum > 0)[..., None], rgb, 0.0))
    exact = R64.exact_mean_rgb_integral()
    _x, mean64, se = R64.estimator(u, v)
    _d, rad, pdf, some = H.sample(T["image"], np.ones(3, f32), u, v)
    x = np.where(some, rad.astype(f64).mean(axis=1) / np.where(some, pdf, 1.0).astype(f64), 0.0)
    print("%s: exact %.6f, host-compiled %.6f, float64 restatement %.6f, standard error %.3e (relative %.2e)"
          % (name, exact, x.mean(), mean64, se, se / exact))
    assert abs(mean64 - exact) <= 5.0 * se  # the restatement itself
    assert abs(x.mean() - exact) <= 5.0 * se


# ---- 6. the importer -------------------------------------------------------------------------------------------------------
def _dome(desc):
    domes = [l for l in desc.lights if l["kind"] == "dome"]
    assert len(domes) == 1
    return domes[0]


def test_importer_decodes_the_environment(crt):
    path = os.path.join(ROOT, "scenes", "domelight.usda")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        desc = crt.usda.load(path, environment_maps=True)
    assert not [w for w in caught if "not decoded" in str(w.message)]
    env = _dome(desc)["environment"]
    assert (env["width"], env["height"]) == (128, 64) and env["rgb"].shape == (64, 128, 3)
    assert np.array_equal(env["rgb"], ec.sky_env(crt))
    m = env["light_to_world"]
    assert np.allclose(m, ec.rotate_y(20.0), atol=1e-6)
    T = crt.Environment(env["width"], env["height"], env["rgb"], m).tables()
    assert np.allclose(T["world_to_light"].astype(f64) @ T["light_to_world"].astype(f64), np.eye(3), atol=1e-6)
    # a description with an environment is plain data: it survives the broadcast of shard.import_once
    back = pickle.loads(pickle.dumps(desc))
    e2 = _dome(back)["environment"]
    assert np.array_equal(e2["rgb"], env["rgb"]) and np.array_equal(e2["light_to_world"], m)
    lights = crt.make_lights(back.lights)
    k = [i for i, l in enumerate(back.lights) if l["kind"] == "dome"][0]
    assert lights[k].kind == crt.LIGHT_DOME_MAP and len(lights._environments) == 1


def test_importer_default_is_unchanged(crt):
    with pytest.warns(UserWarning, match="environment map not decoded, using the uniform colour"):
        desc = crt.usda.load(os.path.join(ROOT, "scenes", "domelight.usda"))
    assert "environment" not in _dome(desc)
    assert crt.make_lights(desc.lights)[[l["kind"] for l in desc.lights].index("dome")].kind == crt.LIGHT_DOME


STAGE = """#usda 1.0
def Xform "World"
{
    def Camera "Cam"
    {
        float focalLength = 28
    }

    def DomeLight "Sky"
    {
        float inputs:intensity = 1.0
        asset inputs:texture:file = @%s@
        %s
    }
}
"""


@pytest.mark.parametrize("file,fmt,message", [
    ("sky_env.exr", 'token inputs:texture:format = "angular"', "not supported"),
    ("missing.exr", "", "could not load"),
    ("sky.png", "", "could not load"),
])
def test_importer_falls_back_to_the_uniform_dome(crt, tmp_path, file, fmt, message):
    import shutil
    shutil.copy(os.path.join(ROOT, "scenes", "sky_env.exr"), tmp_path / "sky_env.exr")
    (tmp_path / "sky.png").write_bytes(b"\x89PNG\r\n\x1a\n")
    stage = tmp_path / "stage.usda"
    stage.write_text(STAGE % (file, fmt))
    with pytest.warns(UserWarning, match=message):
        desc = crt.usda.load(str(stage), environment_maps=True)
    assert "environment" not in _dome(desc)


def test_importer_automatic_format(crt, tmp_path):
    import shutil
    shutil.copy(os.path.join(ROOT, "scenes", "sky_env.exr"), tmp_path / "sky_env.exr")
    stage = tmp_path / "stage.usda"
    stage.write_text(STAGE % ("sky_env.exr", 'token inputs:texture:format = "automatic"'))
    desc = crt.usda.load(str(stage), environment_maps=True)
    assert _dome(desc)["environment"]["width"] == 128


def test_importer_behind_the_crate_reader(crt, tmp_path, monkeypatch):
    """A stage that arrives through the USDC branch of usda.load gets the same dome. No crate with a textured DomeLight
    exists among the samples and none can be written here (the package reads crates, it does not write them), so the
    crate reader's OUTPUT stands in for one: usdc.parse is replaced by a function that returns the Prim trees of the
    same stage, the asset path as the plain token text the crate reader yields for an asset value (usdc.py, T_ASSET) and
    the format as a token's text. What this pins: a file that starts with the crate magic goes through usdc.parse and
    reaches the DomeLight arm with inputs:texture:file / :format read by prim.attr, resolved against the file's directory."""
    import shutil
    shutil.copy(os.path.join(ROOT, "scenes", "sky_env.exr"), tmp_path / "sky_env.exr")
    text = STAGE % ("sky_env.exr", 'token inputs:texture:format = "latlong"\n        float xformOp:rotateY = 20\n'
                    '        uniform token[] xformOpOrder = ["xformOp:rotateY"]')
    seen = []

    def fake_parse(raw):
        seen.append(raw[:8])
        meta, roots = crt.usda.parse(text)
        sky = [p for p in roots[0].children if p.name == "Sky"][0]
        assert sky.attr("inputs:texture:file") == "sky_env.exr"  # plain text, no @...@: the crate reader's form
        return meta, roots
    monkeypatch.setattr(crt.usdc, "parse", fake_parse)
    crate = tmp_path / "stage.usd"
    crate.write_bytes(b"PXR-USDC" + b"\0" * 80)
    desc = crt.usda.load(str(crate), environment_maps=True)
    assert seen == [b"PXR-USDC"]
    env = _dome(desc)["environment"]
    assert (env["width"], env["height"]) == (128, 64) and np.allclose(env["light_to_world"], ec.rotate_y(20.0), atol=1e-6)
    with pytest.warns(UserWarning, match="not decoded"):
        assert "environment" not in _dome(crt.usda.load(str(crate)))


# ---- 7. the C ABI ------------------------------------------------------------------------------------------------------------
def test_abi_refusals_and_the_light_record(crt):
    L = crt.lib()
    px = np.ones(4 * 4 * 3, dtype=f32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for w, h in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        assert not L.crt_environment_new(w, h, fp(px), None)
        assert b"16384" in L.crt_last_error(), (w, h)
    assert not L.crt_environment_new(4, 4, None, None)
    assert b"no pixels" in L.crt_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        q = px.copy()
        q[3 * 5 + 1] = bad
        assert not L.crt_environment_new(4, 4, fp(q), None)
        assert b"texel (1, 1) is not finite" in L.crt_last_error()
    singular = np.array([1, 0, 0, 2, 0, 0, 0, 0, 1], dtype=f32)
    assert not L.crt_environment_new(4, 4, fp(px), fp(singular))
    assert b"inverse" in L.crt_last_error()
    neg = px.copy()
    neg[:3] = -1.0  # negative texels are accepted as upstream
    env = crt.Environment(4, 4, neg)
    assert env.tables()["conditional_func"][0, 0] == 0
    light = crt.CrtLight()
    tint = np.array([0.25, 0.5, 0.75], dtype=f32)
    assert L.crt_light_dome_mapped(C.byref(light), fp(tint), env.h) == 0
    assert light.kind == crt.LIGHT_DOME_MAP == 4 and light.geom_id == 0xFFFFFFFF
    assert list(light.radiance) == [0.25, 0.5, 0.75]
    ident = env.tables()["id"]
    assert np.array([light.center[0]], dtype=f32).view(u32)[0] == ident
    assert 0x00800000 <= ident < 0x7f800000  # the bits of a normal finite float (crt.h)
    assert L.crt_light_dome_mapped(None, fp(tint), env.h) < 0 and L.crt_light_dome_mapped(C.byref(light), fp(tint), None) < 0
    assert C.sizeof(crt.CrtLight) == 84
    for name in ("crt_environment_new", "crt_environment_free", "crt_environment_tables", "crt_light_dome_mapped"):
        assert hasattr(L, name) and name in crt.ABI_SYMBOLS
    # ids: a new environment in a freed slot carries a new generation
    env.free()
    again = crt.Environment(4, 4, px)
    assert again.tables()["id"] != ident


def test_environment_slots_run_out_with_a_reason(crt):
    px = np.ones(3, dtype=f32)
    held = []
    with pytest.raises(crt.CrtError, match="slots"):
        for _ in range(64):
            held.append(crt.Environment(1, 1, px))
    assert 1 <= len(held) <= 16
    del held
    crt.Environment(1, 1, px)  # the slots come back
