"""Round curve segments (Geometry::RoundCurves) without a GPU: the float32 restatement of rounded_cone_intersect
(tests/curve_ref.py) against the reference's known answers and against Quilez's signed distance in float64; the device
function (kernels/traverse.hip.h, rounded_cone) compiled as host C++ against the restatement, bit for bit; the builder, the
C ABI, the device image and the engine selector on curve scenes. The GPU side is tests/test_gpu_curves.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import curve_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("curve_host") / "libcurve_host.so"
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + os.path.join(ROOT, "crust-render_amd", "csrc", "kernels"),
           os.path.join(ROOT, "tests", "host_shade", "curve_host.cpp"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    L = C.CDLL(str(out))
    L.curve_rounded_cone_n.argtypes = [C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]

    def run(rows):
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 16)
        n = len(rows)
        hit, tn, anyh = np.zeros(n, np.int32), np.zeros((n, 4), np.float32), np.zeros(n, np.int32)
        L.curve_rounded_cone_n(rows.ctypes.data_as(C.POINTER(C.c_float)), n, hit.ctypes.data_as(C.POINTER(C.c_int)),
                               tn.ctypes.data_as(C.POINTER(C.c_float)), anyh.ctypes.data_as(C.POINTER(C.c_int)))
        return hit.astype(bool), tn[:, 0], tn[:, 1:4], anyh.astype(bool)
    return run


def _row(o, d, p0, p1, r0, r1, t_min, t_max):
    return np.array(list(o) + list(d) + list(p0) + [r0] + list(p1) + [r1, t_min, t_max], np.float32)


def _both(host):
    """The two implementations under test as row -> (hit, t, n)."""
    def ref(rows):
        return cr.run_pairs(rows)

    def dev(rows):
        return host(rows)[:3]
    return (("restatement", ref), ("device source as host C++", dev))


def test_known_answers_of_the_reference(host):
    """curve.rs:227-306 with the reference's tolerances, on the restatement and on the device function."""
    for who, fn in _both(host):
        for label, o, d, p0, p1, r0, r1, lo, hi, expect in cr.known_answers():
            hit, t, n = fn(_row(o, d, p0, p1, r0, r1, lo, hi)[None, :])
            if expect is None:
                assert not hit[0], (who, label)
                continue
            want_t, t_tol, want_n, n_tol = expect
            assert hit[0], (who, label)
            assert abs(float(t[0]) - want_t) < t_tol, (who, label, float(t[0]))
            if want_n is not None:
                assert np.all(np.abs(n[0] - np.array(want_n, np.float32)) <= n_tol), (who, label, n[0])
        rows = np.stack([_row(o, d, p0, p1, r0, r1, 0.001, np.inf) for o, d, p0, p1, r0, r1 in cr.taper_case()])
        hit, t, _n = fn(rows)
        assert hit.all(), who
        thick, thin = 3.0 - float(t[0]), 3.0 - float(t[1])
        assert thick > thin + 0.2, (who, thick, thin)  # the cone tapers
        assert thick <= 0.5 + 1e-3 and thin >= 0.1 - 1e-3, (who, thick, thin)


def test_edge_list_answers(host):
    """What the edge list must give, whoever computes it: inclusive at t_max, a miss one ulp below, no hit without a
    direction, the same point at any scale of the direction."""
    labels, rows = cr.edge_pairs()
    for who, fn in _both(host):
        hit, t, n = fn(rows)
        got = dict(zip(labels, zip(hit.tolist(), t.tolist())))
        assert got["t_max at the hit"] == (True, 2.5), (who, got["t_max at the hit"])
        assert got["t_min at the hit"] == (True, 2.5), who
        assert not got["t_max one ulp below the hit"][0], who
        assert not got["zero direction"][0] and not got["tiny direction"][0] and not got["behind the origin"][0], who
        assert got["along the axis"] == (True, 2.5), who
        assert got["swallowed cap (d2 <= 0)"][0] and abs(got["swallowed cap (d2 <= 0)"][1] - 4.0) < 1e-3, who
        assert got["p0 == p1"][0] and abs(got["p0 == p1"][1] - 2.5) < 1e-4, who
        assert abs(got["direction x 2"][1] - 1.25) < 1e-3 and abs(got["direction x 1e-3"][1] - 2500.0) < 1.0, who
        assert got["starts inside"][0] and got["starts inside a cap"][0], who
        assert got["r = 0"][0] and abs(got["r = 0"][1] - 3.0) < 1e-3, who  # radii clamp to 1e-6: a hair, not nothing


def test_device_source_equals_the_restatement_bitwise(host):
    """2^16 seeded pairs and the edge list: hit, t and the normal of the device function compiled as host C++ are the
    restatement's bits; its any-hit form answers as the closest-hit form."""
    _labels, edges = cr.edge_pairs()
    rows = np.concatenate([cr.random_pairs(1 << 16, 20261), edges], 0)
    hit, t, n = cr.run_pairs(rows)
    h_hit, h_t, h_n, h_any = host(rows)
    assert 0.25 < hit.mean() < 0.9, hit.mean()  # the corpus exercises both outcomes
    assert np.array_equal(h_hit, hit), np.nonzero(h_hit != hit)[0][:8]
    assert np.array_equal(h_any, hit), np.nonzero(h_any != hit)[0][:8]
    assert np.array_equal(h_t.view(np.uint32), t.view(np.uint32)), np.nonzero(h_t.view(np.uint32) != t.view(np.uint32))[0][:8]
    assert np.array_equal(h_n.view(np.uint32), n.view(np.uint32)), np.nonzero((h_n.view(np.uint32) != n.view(np.uint32)).any(1))[0][:8]


def test_restatement_describes_a_rounded_cone():
    """Quilez's sdRoundCone in float64 at o + t*d: within the reference's own 1e-3 (curve.rs:255) for hits whose incidence
    |n . rd| is at least 0.2, on the reference's test scale; at least half of the hits pass that filter. Rays start
    outside the solid (from inside, the nearest boundary may be an interior sphere surface: curve.rs:12-13)."""
    rows = cr.random_pairs(1 << 15, 77)
    o, d = rows[:, 0:3].astype(np.float64), rows[:, 3:6].astype(np.float64)
    p0, p1, r0, r1 = rows[:, 6:9], rows[:, 10:13], rows[:, 9], rows[:, 13]
    outside = cr.sd_round_cone(o, p0, p1, r0, r1) > 0.01
    rows[:, 15] = np.inf
    hit, t, n = cr.run_pairs(rows)
    use = hit & outside
    assert use.sum() > 8000, use.sum()
    # the outside filter is this test's own addition: it may not eat the corpus (at most a tenth of the hits: a ray of
    # random_pairs starts anywhere in an 8^3 box, a segment with its 0.01 margin fills a small part of it)
    print("hits %d, of them starting outside %d" % (hit.sum(), use.sum()))
    assert use.sum() >= 0.9 * hit.sum(), (use.sum(), hit.sum())
    rd = d / np.linalg.norm(d, axis=1, keepdims=True)
    inc = np.abs((n.astype(np.float64) * rd).sum(1))
    ok = use & (inc >= 0.2)
    assert ok.sum() >= 0.5 * use.sum(), (ok.sum(), use.sum())
    sd = cr.sd_round_cone(o + t.astype(np.float64)[:, None] * d, p0, p1, r0, r1)
    worst = np.abs(sd[ok]).max()
    print("largest |signed distance| at a hit: %.3g over %d hits" % (worst, ok.sum()))
    assert worst <= 1e-3, worst


# ---------------------------------------------------------------- builder and ABI
def _f32_sum(x):
    s = f32(0)
    for v in x:
        s = f32(s + f32(v))
    return s


def test_symbols_are_exported(crt):
    for name in ("crt_attach_round_curves", "crt_set_round_curves"):
        assert hasattr(crt.lib(), name) and name in crt.ABI_SYMBOLS, name
    src = "#include <stdio.h>\n#include \"crt.h\"\nint main(void){printf(\"%zu\\n\", sizeof(CrtCurveSegment));return 0;}\n"
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        assert subprocess.check_output([os.path.join(td, "s")], text=True).strip() == "32"  # scene.rs:15-23


def test_scene_queries_count_curve_segments(crt):
    seg = cr.tuft(257, 11)
    b = crt.SceneBuilder()
    gid = b.attach_round_curves(seg)
    assert gid == 0 and b.count() == 1
    s = b.commit()
    assert s.primitive_count() == 257 and s.geometry_count() == 1
    out = (C.c_size_t * 5)()
    assert crt.lib().crt_scene_primitive_breakdown(s.h, out) == 0 and list(out) == [0, 0, 257, 0, 0]
    assert s.unique_primitive_breakdown()["curve_segments"] == 257
    lo = np.minimum(seg[:, 0:3] - seg[:, 3:4], seg[:, 4:7] - seg[:, 7:8])  # prim.rs:202-206
    hi = np.maximum(seg[:, 0:3] + seg[:, 3:4], seg[:, 4:7] + seg[:, 7:8])
    assert np.array_equal(s.bounds(), np.concatenate([lo.min(0), hi.max(0)]))
    e = hi - lo
    diag = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    se = hi.max(0) - lo.min(0)
    n, scene_d, mean_d, max_d = s.primitive_extents()
    assert n == 257 and f32(max_d) == diag.max()
    assert f32(scene_d) == np.sqrt(f32(f32(se[0] * se[0] + se[1] * se[1]) + se[2] * se[2]))
    assert f32(mean_d) == f32(_f32_sum(diag) / f32(257))
    # instanced: the breakdown of what is resident descends, each prototype once
    top = crt.SceneBuilder()
    top.attach_instance(s, crt.affine(t=(1, 0, 0)))
    top.attach_instance(s, crt.affine(t=(-1, 0, 0)))
    top.attach_sphere((0, 3, 0), 0.5)
    ts = top.commit()
    assert ts.unique_primitive_breakdown() == dict(triangles=0, spheres=1, curve_segments=257, cubic_curve_spans=0, instances=2)
    assert crt.lib().crt_scene_primitive_breakdown(ts.h, out) == 0 and list(out) == [0, 1, 0, 0, 2]


def test_set_round_curves_keeps_the_mask_and_copies(crt):
    seg = cr.tuft(9, 3)
    b = crt.SceneBuilder()
    g0 = b.attach_sphere((0, 0, 0), 1.0, mask=cr.MASK_SHADOW)
    g1 = b.attach_round_curves(seg[:4], mask=cr.MASK_CAMERA)
    b.set_round_curves(g0, seg)  # a sphere slot becomes curves, mask kept
    work = seg[:2].copy()
    b.set_round_curves(g1, work)
    work[:] = 1e9  # the arrays were copied
    with pytest.raises(crt.CrtError) as ei:
        b.set_round_curves(7, seg)
    assert ei.value.code == -2  # CRT_ERR_BAD_ID
    s = b.commit()
    assert s.unique_primitive_breakdown()["curve_segments"] == 11 and s.unique_primitive_breakdown()["spheres"] == 0
    assert np.all(np.abs(s.bounds()) < 10)
    _nodes, _leaves, _packets, _indices, counts = s.tree()
    assert counts["prims"] == 11 and counts["packets"] == 0  # scalar-list primitives, never packed


def test_non_finite_segments_are_refused(crt):
    seg = cr.tuft(5, 3)
    for col, val in ((0, np.nan), (3, np.inf), (6, -np.inf), (7, np.nan)):
        bad = seg.copy()
        bad[2, col] = val
        b = crt.SceneBuilder()
        with pytest.raises(crt.CrtError) as ei:
            b.attach_round_curves(bad)
        assert ei.value.code == -1 and b"segment 2" in crt.lib().crt_last_error(), crt.lib().crt_last_error()
        assert b.count() == 0
        g = b.attach_round_curves(seg)
        with pytest.raises(crt.CrtError) as ei:
            b.set_round_curves(g, bad)
        assert ei.value.code == -1
        assert b.commit().primitive_count() == 5  # the slot kept its geometry
    assert crt.lib().crt_attach_round_curves(None, None, 0, 0, None) == -1


SCENES = {"one": cr.scene_one, "curve_only": lambda: _curve_only(), "tuft": cr.scene_tuft, "instanced": cr.scene_instanced}


def _curve_only():
    s = cr.RefScene()
    s.curves(cr.tuft(40, 5))
    return s


@pytest.mark.parametrize("direct", ["0", "1"])
@pytest.mark.parametrize("name", list(SCENES))
def test_image_and_engine_selection_of_curve_scenes(crt, monkeypatch, name, direct):
    """The device image of curve-only, mixed and instanced-curve scenes passes its self-check with direct leaf words on and
    off; the selector never gives such an image a four-wave instance and asks for the kernels with the curve arm."""
    monkeypatch.setenv("CRT_DIRECT_LEAVES", direct)
    monkeypatch.delenv("CRT_WIDE", raising=False)
    s = SCENES[name]().build(crt)
    chk = s.image_check()
    assert chk["direct_leaves"] == int(direct)
    if direct == "1":
        assert chk["leaf_words_direct_index"] > 0, chk  # leaves of one to three segments go into the child word
    else:
        assert chk["leaf_words_direct_index"] == 0 and chk["leaf_words_direct_instance"] == 0, chk
    if name == "one":
        assert chk["nodes"] == 1
    for want in (-1, 0, -2, -3, -4):
        sel = s.engine_select(want)
        assert sel["wide"] == 0 and sel["direct"] == int(direct), (want, sel)
        assert sel["cold"] & 16 and sel["cold"] & 2, sel      # the curve bit, and the pending normal it implies
        assert sel["ext_cold"] == 23 and sel["path_cold"] == 23, sel
    for want in (1, 2):
        with pytest.raises(crt.CrtError) as ei:
            s.engine_select(want)
        assert ei.value.code == -5  # CRT_ERR_UNSUPPORTED
    for wide in ("1", "2"):  # the A/B request falls back
        monkeypatch.setenv("CRT_WIDE", wide)
        for want in (-2, -3):
            assert s.engine_select(want)["wide"] == 0


def test_scenes_without_curves_select_as_before(crt, monkeypatch):
    monkeypatch.delenv("CRT_WIDE", raising=False)
    b = crt.SceneBuilder()
    b.attach_triangles(*cr.FLOOR)
    b.attach_sphere((0, 1, 0), 0.5)
    sel = b.commit().engine_select(-1)
    assert sel["cold"] & 16 == 0 and sel["ext_cold"] & 16 == 0 and sel["path_cold"] & 16 == 0 and sel["wide"] == 1, sel


# ---------------------------------------------------------------- the brute-force query's own condition
@pytest.mark.parametrize("name", ["one", "tuft", "instanced"])
def test_undecided_rays_stay_under_the_cap(oracle, name):
    """Condition on the seeds of tests/test_gpu_curves.py: at most 1 % of a test's rays are undecided (a runner-up within
    8 ulp of the winner), for every t range the GPU tests run."""
    import gpu_curve_cases as gc
    for k, (lo, hi) in enumerate(cr.T_RANGES):
        ref = gc.reference(oracle, name, k)
        und = float((~ref["decided"]).mean())
        print(name, (lo, hi), "undecided %.4f, hit %.3f, occluded %.3f" % (und, ref["hit"].mean(), ref["occluded"].mean()))
        assert und <= cr.UNDECIDED_CAP, (name, lo, hi, und)
        if hi == float("inf"):
            assert ref["hit"].mean() > 0.2  # the rays do meet the scene
