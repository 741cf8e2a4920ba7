"""The two material views of kernels/shade.hip.h give the same bits, WITHOUT a GPU: the shading functions compiled as
host C++ (tests/host_shade/derived_host.cpp) over MatRaw — every per-material constant computed at the call, what the seam
entry points run — and over MatDerived — the constants read from the DevMaterial record that derive_material() fills once
per renderer, what the shade kernels of simple-material scenes run — compared record by record with each other and with
the oracle's functions: the 12 lobe classes of seam_cases (20 000 calls per class and method, as
test_shading_seam_host.py runs them) and degenerate records (all weights 0, metalness 1, roughness 0 and 1, anisotropy 1,
ior 1). Classes a simple-material table can hold are also run through the SIMPLE instantiation of either view, the one
the bench's kernels are built from. The GPU side of the same statement is tests/test_gpu_mat_derived.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import seam_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000  # calls per lobe class and method
SIMPLE_CLASSES = ("base", "metal", "anisotropic", "emissive")  # no coat, fuzz, thin film, transmission or subsurface


class ViewDrivers:
    """scatter / eval / emitted of one instantiation (prefix raw, drv, sraw, sdrv) of derived_host.cpp."""

    def __init__(self, cdll, prefix):
        self.L, self.prefix = cdll, prefix
        for name in ("scatter_n", "eval_n", "emitted_n"):
            f = getattr(cdll, "%s_%s" % (prefix, name))
            f.restype = None
            f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]

    def _run(self, name, table, queries, out_dtype, per=1):
        table, queries = np.ascontiguousarray(table), np.ascontiguousarray(queries)
        out = np.zeros(len(queries) * per, dtype=out_dtype)
        getattr(self.L, "%s_%s" % (self.prefix, name))(table.ctypes.data, len(table), queries.ctypes.data, len(queries), out.ctypes.data)
        return out

    def scatter(self, mats, q): return self._run("scatter_n", mats, q, sc.SCATTER_SAMPLE)
    def eval(self, mats, q): return self._run("eval_n", mats, q, sc.BSDF_EVAL)
    def emitted(self, mats, q): return self._run("emitted_n", mats, q, np.float32, 3).reshape(-1, 3)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("derived_host") / "libderived_host.so"
    k = os.path.join(ROOT, "crust-render_amd", "csrc", "kernels")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + k,
           os.path.join(ROOT, "tests", "host_shade", "derived_host.cpp"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return C.CDLL(str(out))


@pytest.fixture(scope="module")
def views(lib):
    return {p: ViewDrivers(lib, p) for p in ("raw", "drv", "sraw", "sdrv")}


@pytest.fixture(scope="module")
def oracle():
    return sc.oracle_drivers()


def check_all_equal(views, oracle, mats, q, simple, what):
    """Every method: derived view == raw view == oracle, bit for bit; with `simple`, the SIMPLE instantiations too."""
    for name in ("scatter", "eval", "emitted"):
        want = getattr(oracle, name)(mats, q)
        for prefix in ("raw", "drv") + (("sraw", "sdrv") if simple else ()):
            got = getattr(views[prefix], name)(mats, q)
            bad = sc.mismatches(got, want)
            assert len(bad) == 0, (what, name, prefix, len(bad), got[bad[:2]], want[bad[:2]], q[bad[:2]], mats[q["material"][bad[:2]]])


@pytest.mark.parametrize("cls", sc.CLASSES)
def test_derived_view_equals_raw_view_and_oracle(views, oracle, cls):
    rng = np.random.default_rng(1000 + sc.CLASSES.index(cls))  # the cases test_shading_seam_host.py runs
    mats = sc.materials(cls, 257, rng)
    q = sc.shade_queries(N, len(mats), rng)
    check_all_equal(views, oracle, mats, q, cls in SIMPLE_CLASSES, cls)
    if cls != "emissive":  # the calls do reach the lobes (what they reach per class: test_shading_seam_host.py)
        assert views["drv"].scatter(mats, q)["some"].mean() > 0.5 and views["drv"].eval(mats, q)["some"].mean() > 0.8


WEIGHTS = ("base_weight", "specular_weight", "transmission_weight", "subsurface_weight", "fuzz_weight", "coat_weight",
           "thin_film_weight")
DEGENERATE = {
    "all_weights_0": {w: 0.0 for w in WEIGHTS},
    "metalness_1": {"base_metalness": 1.0},
    "roughness_0": {"specular_roughness": 0.0, "coat_roughness": 0.0, "base_diffuse_roughness": 0.0, "fuzz_roughness": 0.0},
    "roughness_1": {"specular_roughness": 1.0, "coat_roughness": 1.0, "base_diffuse_roughness": 1.0, "fuzz_roughness": 1.0},
    "anisotropy_1": {"specular_roughness_anisotropy": 1.0, "coat_roughness_anisotropy": 1.0},
    "ior_1": {"specular_ior": 1.0, "coat_ior": 1.0},
}


@pytest.mark.parametrize("case", sorted(DEGENERATE))
@pytest.mark.parametrize("cls", ("base", "metal", "everything"))
def test_degenerate_records(views, oracle, cls, case):
    rng = np.random.default_rng(7000 + 10 * sorted(DEGENERATE).index(case) + ("base", "metal", "everything").index(cls))
    mats = sc.materials(cls, 64, rng)
    for field, value in DEGENERATE[case].items():
        mats[field] = np.float32(value)
    q = sc.shade_queries(N, len(mats), rng)
    simple = cls != "everything" and not (mats["transmission_weight"] > 0).any()
    check_all_equal(views, oracle, mats, q, simple, (cls, case))


def test_derived_record_layout(lib):
    """A DevMaterial is as large as a CrtMaterial (the shade kernels stage either table under one LDS budget), and a
    finite material derives to finite numbers."""
    rng = np.random.default_rng(3)
    mats = np.concatenate([sc.materials(c, 32, rng) for c in ("base", "metal", "anisotropic", "everything")])
    words = np.zeros(len(mats) * sc.MATERIAL.itemsize // 4, dtype=np.uint32)
    lib.derive_n.restype = C.c_size_t
    lib.derive_n.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    assert lib.derive_n(mats.ctypes.data, len(mats), words.ctypes.data) == sc.MATERIAL.itemsize
    rec = words.reshape(len(mats), -1)
    assert (rec[:, 0] == mats["kind"]).all()
    assert np.isfinite(rec[:, 1:].view(np.float32)).all()
    pmf = rec[:, 4:9].view(np.float32)  # the five lobe masses sum to 1
    assert np.allclose(pmf.sum(axis=1), 1.0, atol=1e-6) and (pmf >= 0).all()
