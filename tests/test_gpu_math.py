"""The deterministic math, the sampler and the bare arithmetic ON gfx950, function by function: tests/host_shade/math_dev.hip
(one small kernel per function of kernels/dmath.hip.h and kernels/qmc.hip.h, built here with the product's own flags) run
over tests/math_cases.py and compared BIT FOR BIT with the oracle's drivers (oracle/ora_mathdrv.c); the oracle itself is
judged against libm / mpmath in tests/test_math_host.py. The primitive kernels — f32 and f64 + - x / sqrt, dot,
normalize, the conversions and rint — are compared with numpy on the host: the first check of the premise "correctly
rounded on host and gfx950, denormals on"  against something that is not this project's code.
One process, one device context, no retries."""
import numpy as np
import pytest

import math_cases as mc
import math_drivers as md
import seam_cases as sc
from math_cases import assert_same

pytestmark = pytest.mark.gpu
U = np.uint32


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    return md.device(tmp_path_factory.mktemp("math_dev"))


@pytest.fixture(scope="module")
def ora():
    return md.oracle()


@pytest.fixture(scope="module")
def X():
    return mc.unary()


@pytest.mark.parametrize("name", ["sincos", "cos", "acos", "exp", "log"])
def test_unary_functions_match_the_oracle_on_every_case(dev, ora, X, name):
    got, want = dev(name, X), ora(name, X)
    for g, w in zip(got if name == "sincos" else [got], want if name == "sincos" else [want]):
        assert_same(g, w, name, X)
    if name == "sincos":  # defined for every f32: the out-of-domain rule holds on the device as stated
        with np.errstate(invalid="ignore"):
            big = np.abs(X.astype(np.float64)) >= 2.0 ** 62
        assert (got[0][big] == 0).all() and (got[1][big] == 1).all() and np.isinf(X[big]).any()
        assert np.isnan(got[0][np.isnan(X)]).all() and np.isfinite(got[0][~big & ~np.isnan(X)]).all()


def test_pow_matches_the_oracle_on_every_case(dev, ora):
    for x, y in (mc.pow_bulk(), mc.pow_specials()):
        assert_same(dev("pow", x, y), ora("pow", x, y), "pow", x, y)


def test_min_max_clamp_helpers_match_the_oracle_on_the_nan_zero_cross_product(dev, ora):
    (a, b), (x, lo, hi) = mc.minmax_cross()
    for name in ("rmax", "rmin", "smax", "smin"):
        got, want = dev(name, a, b), ora(name, a, b)
        # a NaN result must be a NaN on both sides; everything else, the sign of a zero included, the same bits
        assert_same(got, want, name, a, b)
    assert_same(dev("rclamp", x, lo, hi), ora("rclamp", x, lo, hi), "rclamp", x, lo, hi)
    assert np.isnan(a).any() and np.isnan(b).any() and (np.signbit(a) & (a == 0)).any()


def test_sampler_functions_and_tables_match_the_oracle(dev, ora):
    rng = np.random.default_rng(41)
    n = 1 << 24
    a, b = (rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(U) for _ in range(2))
    a[:4], b[:4] = [0, 0xffffffff, 1, 0x80000000], [0, 0xffffffff, 0xffff0000, 1]
    m = 1 << 20
    for name, args in (("draw_sample4", (a, b)), ("draw_rnd1", (a, b)), ("pcg_hash", (a[:m],)),
                       ("laine_karras", (a[:m], b[:m])), ("owen", (a[:m], b[:m])), ("unit_f32", (a[:m],)),
                       ("new_domain", (a[:m], b[:m].view(np.int32))),
                       ("sampler_new", (rng.integers(-2 ** 31, 2 ** 31, size=(m, 4)).astype(np.int32),))):
        assert_same(dev(name, *args), ora(name, *args), name, *args)
    pats = mc.sampler_patterns(ora)[:64]
    N = (1 << 16) + 1
    p, i = np.repeat(pats, N), np.tile(np.arange(N, dtype=U), len(pats))
    got = dev("draw_sample4", p, i)
    assert_same(got, ora("draw_sample4", p, i), "draw_sample4 by index", p, i)
    assert_same(dev("draw_rnd1", p, i), ora("draw_rnd1", p, i), "draw_rnd1 by index", p, i)
    assert (got >= 0).all() and (got < 1).all() and len(pats) == 64
    assert np.array_equal(dev.table("sobol_dirs"), ora.table("sobol_dirs"))
    assert np.array_equal(dev.table("sobol_table"), ora.table("sobol_table"))  # filled in LDS by the block, as in k_shade


# ---- the premise: one correctly rounded IEEE operation per written operation, denormals on ------------------------------
N_PRIM = 1 << 24


def test_f32_arithmetic_is_correctly_rounded_with_denormals(dev):
    mc.check_f32_arithmetic(dev, N_PRIM)


def test_f64_arithmetic_conversion_and_rint_are_correctly_rounded_with_denormals(dev):
    mc.check_f64_arithmetic(dev, N_PRIM)


def test_dot_and_normalize_are_the_written_sequence(dev):
    mc.check_dot_and_normalize(dev, N_PRIM // 4)


# ---- the reachable input of the conversion defect ----------------------------------------------------------------------
def test_thin_film_of_any_authored_thickness_matches_the_oracle_through_the_seam(crt):
    """thin_film_thickness is authored and unclamped (usda.py) and feeds cos_det(2 pi 2 eta thickness cos / lambda): at 1e18
    the phase is past the range of the double -> int64 conversion sincos_det used to make, where x86 and gfx950 answered
    with different quadrants. crt_material_eval_n against the oracle: finite, and the same bits."""
    mats, q = mc.thin_film_cases(sc)
    table = crt.shading.DeviceMaterials([crt.CrtMaterial.from_buffer_copy(m.tobytes()) for m in mats])
    got = table.eval(crt.shading.to_device(q)).cpu().numpy().view(sc.BSDF_EVAL)
    mc.check_thin_film(sc, mats, q, got, sc.oracle_drivers().eval(mats, q))
