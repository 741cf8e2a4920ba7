"""Cubic curve spans (Geometry::CubicCurves) without a GPU: the float32 truth of tests/cubic_ref.py against the
reference's known answers (curve.rs:310-415) and its own literal recursion; the flatness depth against float64; the
device source of the intersector compiled as host C++ (tests/host_shade/cubic_host.cpp) bit for bit against the truth;
the builder, the ABI, the device image and the engine selection; the USD reader's basis conversion; and the condition
every GPU test's rays are held to — at most 1 % of them undecided. The GPU side is tests/test_gpu_cubic_curves.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cubic_ref as cu
import curve_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """cubic_span<false / true> and cubic_flatness_depth as host C++: the flags of tests/test_curves.py's curve_host."""
    out = tmp_path_factory.mktemp("cubic_host") / "libcubic_host.so"
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + os.path.join(ROOT, "crust-render_amd", "csrc", "kernels"),
           os.path.join(ROOT, "tests", "host_shade", "cubic_host.cpp"),
           os.path.join(ROOT, "crust-render_amd", "csrc", "bvh_build.cpp"), "-o", str(out), "-lpthread"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    L = C.CDLL(str(out))
    fp, up, ip = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    L.cubic_span_n.argtypes = [fp, up, C.c_size_t, ip, fp, ip]
    L.cubic_flatness_depth_n.argtypes = [fp, fp, C.c_size_t, up]

    class Host:
        @staticmethod
        def span(rows, depth=None):
            rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 22)
            n = len(rows)
            depth = Host.depth(rows[:, 6:18], f32(2.0) * np.maximum(rows[:, 18], rows[:, 19])) if depth is None else depth
            depth = np.ascontiguousarray(np.broadcast_to(depth, (n,)), np.uint32)
            hit, tn, anyh = np.zeros(n, np.int32), np.zeros((n, 4), np.float32), np.zeros(n, np.int32)
            L.cubic_span_n(rows.ctypes.data_as(fp), depth.ctypes.data_as(up), n, hit.ctypes.data_as(ip), tn.ctypes.data_as(fp),
                           anyh.ctypes.data_as(ip))
            return hit.astype(bool), tn[:, 0], tn[:, 1:4], anyh.astype(bool)

        @staticmethod
        def depth(cp, max_width):
            cp = np.ascontiguousarray(cp, np.float32).reshape(-1, 12)
            mw = np.ascontiguousarray(np.broadcast_to(np.asarray(max_width, np.float32), (len(cp),)), np.float32)
            out = np.zeros(len(cp), np.uint32)
            L.cubic_flatness_depth_n(cp.ctypes.data_as(fp), mw.ctypes.data_as(fp), len(cp), out.ctypes.data_as(up))
            return out
    return Host


def _row(o, d, cp, r0, r1, t_min=0.001, t_max=INF):
    return np.array(list(o) + list(d) + list(np.asarray(cp, np.float32).reshape(-1)) + [r0, r1, t_min, t_max], np.float32)


def _both(host):
    return (("restatement", lambda rows: cu.run_pairs(rows)), ("device source as host C++", lambda rows: host.span(rows)[:3]))


# ---------------------------------------------------------------- the reference's known answers
def test_known_answers_of_the_reference(host):
    """curve.rs:310-415, the cubic_curve_tests module, with the reference's tolerances — on the literal recursion, on the
    vectorised walk and on the device function; the two depth tests on the restated and on the host's depth function."""
    straight, quarter = cu.straight_cp(), np.asarray(cu.QUARTER, np.float32)
    for who, depth in (("restatement", lambda cp, w: int(cu.flatness_depth(cp, f32(w)))), ("host", lambda cp, w: int(host.depth(cp, w)[0]))):
        assert depth(straight, 1.0) == 0, who            # flat_span_needs_no_subdivision
        assert depth(quarter, 0.1) > 0, (who, depth(quarter, 0.1))  # curved_span_requires_subdivision
    o, d = (2, 3, 0), (0, -1, 0)
    s2 = float(np.sqrt(f32(2.0)) / f32(2.0))

    def literal(rows):
        out = [cu.cubic_curve_intersect(r[0:3], r[3:6], r[6:18], r[18], r[19], r[20], r[21]) for r in rows]
        return (np.array([x is not None for x in out]), np.array([0.0 if x is None else x[0] for x in out], np.float32),
                np.array([[0, 0, 0] if x is None else x[1] for x in out], np.float32))
    for who, fn in (("literal recursion", literal),) + _both(host):
        # straight_span_matches_rounded_cone
        hit, t, n = fn(_row(o, d, straight, 0.5, 0.5)[None])
        chit, ct, cn = cr.rounded_cone(np.array(o, np.float32), np.array(d, np.float32), straight[0], straight[3], f32(0.5), f32(0.5), f32(0.001), f32(INF))
        assert hit[0] and bool(chit), who
        assert abs(float(t[0]) - float(ct)) < 1e-4 and np.all(np.abs(n[0] - cn) <= 1e-4), (who, t[0], ct)
        # quarter_circle_arc_is_followed_not_its_chord
        assert fn(_row((s2, s2, 10), (0, 0, -1), quarter, 0.05, 0.05)[None])[0][0], who
        assert not fn(_row((0.5, 0.5, 10), (0, 0, -1), quarter, 0.05, 0.05)[None])[0][0], who
        # ray_passing_wide_misses, respects_t_range
        assert not fn(_row((2, 3, 2), d, straight, 0.5, 0.5)[None])[0][0], who
        assert not fn(_row(o, d, straight, 0.5, 0.5, 0.001, 2.0)[None])[0][0], who


def test_edge_list_answers(host):
    """What the edge list must give, whoever computes it."""
    labels, rows = cu.edge_pairs()
    depth = dict(zip(labels, cu.span_depths(rows[:, 6:20]).tolist()))
    assert depth["depth 10, a miss"] == 10 and depth["all points equal"] == 0 and depth["straight span"] == 0, depth
    assert depth["arc point, down the z axis (dx = dy = 0: inf * finite, no NaN)"] >= 2
    for who, fn in _both(host):
        hit, t, n = fn(rows)
        got = dict(zip(labels, zip(hit.tolist(), t.tolist())))
        for k in ("zero direction", "tiny direction", "chord midpoint misses", "t_max before the hit", "depth 10, a miss"):
            assert not got[k][0], (who, k)
        for k in ("axis-parallel, on the first half's x face, hits in the second half",
                  "axis-parallel, on the second half's x face, hits in the first half", "starts inside the tube", "r0 != r1",
                  "depth 10, aimed at the curve's middle", "depth 10, aimed at u = 0.3, slanted"):
            assert got[k][0], (who, k)
        assert abs(got["all points equal"][1] - 2.5) < 1e-4 and abs(got["straight span"][1] - 2.5) < 1e-4, who
        assert abs(got["t_min behind the first hit: the far side"][1] - 10.05) < 1e-3, who
        assert abs(got["depth 10, aimed at the curve's middle"][1] - 5.0) < 1e-2, who
        # unit normals — where the radius is not lost in the rounding of the cap's discriminant (m3 * m3 - m5 + r * r with
        # r = 1e-4 five units away: the depth-10 hair's hits are the reference's arithmetic, bits and all, not geometry)
        thick = hit & (np.minimum(rows[:, 18], rows[:, 19]) >= 0.01)
        nn = np.sqrt((n[thick].astype(np.float64) ** 2).sum(1))
        assert thick.sum() >= 10 and np.all(np.abs(nn - 1) < 1e-5), who


def test_vectorised_walk_equals_the_literal_recursion_bitwise():
    """cubic_span_pairs — what the brute-force query runs on — against the literal recursion: the edge list and 3 000
    seeded pairs, every output bit."""
    _labels, edges = cu.edge_pairs()
    rows = np.concatenate([cu.random_pairs(3000, 901), edges], 0)
    hit, t, n = cu.run_pairs(rows)
    assert 0.2 < hit.mean() < 0.9, hit.mean()
    for i, r in enumerate(rows):
        lit = cu.cubic_curve_intersect(r[0:3], r[3:6], r[6:18], r[18], r[19], r[20], r[21])
        assert (lit is not None) == bool(hit[i]), i
        if lit is not None:
            assert lit[0].view(np.uint32) == t[i].view(np.uint32) and np.array_equal(lit[1].view(np.uint32), n[i].view(np.uint32)), i


# ---------------------------------------------------------------- the flatness depth
def test_depth_against_float64(host):
    """100 000 seeded spans: the depth equals floor(log2(x) / 2) evaluated in float64 on the float32 x, clamped to
    [0, 10], except where x lies within 2 ulp of a power of 4 — there float64's log2 of the float32 x is still exact
    enough to agree, so in practice no exception occurs; the test allows fewer than 0.1 % and requires every one of them
    to be such a boundary case. The host function (bvh_build.cpp) gives the restatement's depth for every span."""
    rng = np.random.default_rng(4242)
    n = 100000
    sp = cu.random_spans(n, rng, bends=(0.0, 1e-4, 0.01, 0.1, 0.5, 2.0), rmin=1e-5, rmax=0.3)
    sp[: n // 10, 12:14] *= f32(1e-3)  # hairs: the clamp at 10
    cp = sp[:, 0:12].reshape(-1, 4, 3)
    mw = f32(2.0) * np.maximum(sp[:, 12], sp[:, 13])
    depth = cu.flatness_depth(cp, mw)
    _l0, x = cu.flatness_x(cp, mw)
    with np.errstate(all="ignore"):
        want = np.clip(np.floor(np.log2(x.astype(np.float64)) / 2.0), 0, 10)
    want = np.where((x >= 1) & np.isfinite(x), want, 0).astype(np.uint32)
    diff = depth != want
    pow4 = np.float32(4.0) ** np.arange(0, 16, dtype=np.float32)
    near = np.zeros(n, bool)
    for p in pow4:
        near |= np.abs(cr._ordered(x) - cr._ordered(np.full(n, p, np.float32))) <= 2
    print("depth histogram", np.bincount(depth, minlength=11).tolist(), "differences from float64", int(diff.sum()), "near a power of 4", int(near.sum()))
    assert diff.sum() < n // 1000 and np.all(near[diff]), (int(diff.sum()), np.nonzero(diff & ~near)[0][:5])
    assert np.bincount(depth, minlength=11).min() > 0  # every depth 0..10 occurs, the clamp included
    assert (x[depth == 10] >= f32(4.0) ** 11).any()      # ... and really clamps
    assert np.array_equal(host.depth(cp, mw), depth)
    # the four zero cases: l0 <= 0, max_width <= 0, x not finite, x < 1
    q = np.asarray(cu.QUARTER, np.float32)
    same = np.tile(np.array([[1, 2, 3]], np.float32), (4, 1))
    cases = [(same, 0.1), (cu.straight_cp() * f32(0.75), 0.1), (q, 0.0), (q, -1.0), (q, 1e-45), (q * f32(1e-3), 1.0)]
    for c, w in cases:
        assert int(cu.flatness_depth(c, f32(w))) == 0 and int(host.depth(c, w)[0]) == 0, (c, w)
    _l, xs = cu.flatness_x(np.stack([c for c, _ in cases]), np.array([w for _, w in cases], np.float32))
    assert not np.isfinite(xs[4]) and 0 < xs[5] < 1, xs
    # on a power of 4 exactly, and one ulp to either side: the exponent rule is exact where a rounded log2f need not be
    for k in (1, 2, 5, 9):
        p = f32(4.0) ** k
        for v, d in ((p, k), (np.nextafter(p, f32(0)), k - 1), (np.nextafter(p, f32(np.inf)), k)):
            # a span whose x IS v: l0 = v * 8 * eps / (SQRT_2 * 6) does not round back in general, so ask the rule itself
            m, e = np.frexp(v)
            assert (int(e) - 1) // 2 == d, (v, d)


# ---------------------------------------------------------------- the device source, compiled for the host
def test_device_source_equals_the_restatement_bitwise(host):
    """The edge list and 20 000 seeded pairs with depths 0-5: hit, t and the normal of cubic_span<false> compiled as host
    C++ are the restatement's bits, cubic_span<true> answers as the closest-hit form; and the depth the host derives is the
    restatement's for every span."""
    labels, edges = cu.edge_pairs()
    rows = np.concatenate([cu.random_pairs(20000, 20262), edges], 0)
    depth = cu.span_depths(rows[:, 6:20])
    assert set(np.unique(depth[:20000]).tolist()) == {0, 1, 2, 3, 4, 5}, np.bincount(depth)
    assert np.array_equal(host.depth(rows[:, 6:18], f32(2.0) * np.maximum(rows[:, 18], rows[:, 19])), depth)
    hit, t, n = cu.run_pairs(rows, depth)
    h_hit, h_t, h_n, h_any = host.span(rows, depth)
    assert 0.2 < hit.mean() < 0.9, hit.mean()
    assert np.array_equal(h_hit, hit), np.nonzero(h_hit != hit)[0][:8]
    assert np.array_equal(h_any, hit), np.nonzero(h_any != hit)[0][:8]
    assert np.array_equal(h_t.view(np.uint32), t.view(np.uint32)), np.nonzero(h_t.view(np.uint32) != t.view(np.uint32))[0][:8]
    assert np.array_equal(h_n.view(np.uint32), n.view(np.uint32)), np.nonzero((h_n.view(np.uint32) != n.view(np.uint32)).any(1))[0][:8]
    # a depth a record could only hold by corruption is clamped, and the walk still ends: the counter bounds it
    wild = host.span(edges, np.full(len(edges), 0xFFFFFFFF, np.uint32))
    ten = host.span(edges, np.full(len(edges), 10, np.uint32))
    assert all(np.array_equal(a, b) for a, b in zip(wild, ten))


# ---------------------------------------------------------------- builder and ABI
def _f32_sum(x):
    s = f32(0)
    for v in x:
        s = f32(s + f32(v))
    return s


def test_symbols_are_exported(crt):
    for name in ("crt_attach_cubic_curves", "crt_set_cubic_curves"):
        assert hasattr(crt.lib(), name) and name in crt.ABI_SYMBOLS, name
    src = "#include <stdio.h>\n#include \"crt.h\"\nint main(void){printf(\"%zu\\n\", sizeof(CrtCubicCurveSegment));return 0;}\n"
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        assert subprocess.check_output([os.path.join(td, "s")], text=True).strip() == "56"  # scene.rs:70-80


def test_scene_queries_count_cubic_spans(crt):
    sp = cu.span_tuft(64, 21)
    b = crt.SceneBuilder()
    gid = b.attach_cubic_curves(sp)
    assert gid == 0 and b.count() == 1
    s = b.commit()
    assert s.primitive_count() == 64 and s.geometry_count() == 1
    out = (C.c_size_t * 5)()
    assert crt.lib().crt_scene_primitive_breakdown(s.h, out) == 0 and list(out) == [0, 0, 0, 64, 0]
    assert s.unique_primitive_breakdown()["cubic_curve_spans"] == 64
    cp = sp[:, 0:12].reshape(-1, 4, 3)
    r = np.maximum(sp[:, 12], sp[:, 13])[:, None]  # prim.rs:246-253
    lo, hi = cp.min(1) - r, cp.max(1) + r
    assert np.array_equal(s.bounds(), np.concatenate([lo.min(0), hi.max(0)]))
    e = hi - lo
    diag = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    se = hi.max(0) - lo.min(0)
    n, scene_d, mean_d, max_d = s.primitive_extents()
    assert n == 64 and f32(max_d) == diag.max()
    assert f32(scene_d) == np.sqrt(f32(f32(se[0] * se[0] + se[1] * se[1]) + se[2] * se[2]))
    assert f32(mean_d) == f32(_f32_sum(diag) / f32(64))
    _nodes, _leaves, _packets, _indices, counts = s.tree()
    assert counts["prims"] == 64 and counts["packets"] == 0  # scalar-list primitives, never packed
    # instanced: the breakdown of what is resident descends, each prototype once
    top = crt.SceneBuilder()
    top.attach_instance(s, crt.affine(t=(1, 0, 0)))
    top.attach_instance(s, crt.affine(t=(-1, 0, 0)))
    top.attach_sphere((0, 3, 0), 0.5)
    top.attach_round_curves(cr.tuft(5, 3))
    ts = top.commit()
    assert ts.unique_primitive_breakdown() == dict(triangles=0, spheres=1, curve_segments=5, cubic_curve_spans=64, instances=2)
    assert crt.lib().crt_scene_primitive_breakdown(ts.h, out) == 0 and list(out) == [0, 1, 5, 0, 2]


def test_set_cubic_curves_keeps_the_mask_and_copies(crt):
    sp = cu.span_tuft(9, 3)
    b = crt.SceneBuilder()
    g0 = b.attach_sphere((0, 0, 0), 1.0, mask=cu.MASK_SHADOW)
    g1 = b.attach_cubic_curves(sp[:4], mask=cu.MASK_CAMERA)
    b.set_cubic_curves(g0, sp)  # a sphere slot becomes spans, mask kept
    work = sp[:2].copy()
    b.set_cubic_curves(g1, work)
    work[:] = 1e9  # the arrays were copied
    with pytest.raises(crt.CrtError) as ei:
        b.set_cubic_curves(7, sp)
    assert ei.value.code == -2  # CRT_ERR_BAD_ID
    s = b.commit()
    bd = s.unique_primitive_breakdown()
    assert bd["cubic_curve_spans"] == 11 and bd["spheres"] == 0, bd
    assert np.all(np.abs(s.bounds()) < 10)
    # the masks: geometry 0 answers shadow rays only, geometry 1 camera rays only (the host image's primitive records)
    w = s.image_prims()  # [n, 16] words: kind, geom_id, prim_id, mask, d[12]
    spans, tails = w[w[:, 0] == 4], w[w[:, 0] == 5]
    assert len(spans) == 11 and len(tails) == 11 and len(w) == 22  # a span is two records, the second behind the first
    assert np.array_equal(np.nonzero(w[:, 0] == 5)[0], np.nonzero(w[:, 0] == 4)[0] + 1)
    assert set(spans[spans[:, 1] == 0][:, 3].tolist()) == {cu.MASK_SHADOW} and set(spans[spans[:, 1] == 1][:, 3].tolist()) == {cu.MASK_CAMERA}
    assert np.array_equal(spans[spans[:, 1] == 0][:, 4:16].view(np.float32), sp[:, 0:12])
    assert np.array_equal(tails[tails[:, 1] == 0][:, 4:6].view(np.float32), sp[:, 12:14])
    assert np.array_equal(tails[tails[:, 1] == 0][:, 6], cu.span_depths(sp))


def test_non_finite_spans_are_refused(crt):
    sp = cu.span_tuft(5, 3)
    for col in range(14):
        bad = sp.copy()
        bad[2, col] = (np.nan, np.inf, -np.inf)[col % 3]
        b = crt.SceneBuilder()
        with pytest.raises(crt.CrtError) as ei:
            b.attach_cubic_curves(bad)
        assert ei.value.code == -1 and b"span 2" in crt.lib().crt_last_error(), crt.lib().crt_last_error()
        assert (b"radius" if col >= 12 else b"control point") in crt.lib().crt_last_error()
        assert b.count() == 0
        g = b.attach_cubic_curves(sp)
        with pytest.raises(crt.CrtError) as ei:
            b.set_cubic_curves(g, bad)
        assert ei.value.code == -1
        assert b.commit().primitive_count() == 5  # the slot kept its geometry
    assert crt.lib().crt_attach_cubic_curves(None, None, 0, 0, None) == -1
    assert crt.lib().crt_set_cubic_curves(None, 0, None, 0) == -1


# ---------------------------------------------------------------- image and engine selection
def _cubic_only():
    s = cu.CubicRefScene()
    s.cubic(cu.span_tuft(40, 5))
    return s


SCENES = {"one": cu.scene_one, "cubic_only": _cubic_only, "tuft": cu.scene_tuft, "mixed": cu.scene_mixed,
          "instanced": cu.scene_instanced, "deep": cu.scene_deep}


@pytest.mark.parametrize("direct", ["0", "1"])
@pytest.mark.parametrize("name", list(SCENES))
def test_image_and_engine_selection_of_cubic_scenes(crt, monkeypatch, name, direct):
    """The device image of cubic-only, cubic + round + sphere + triangle and instanced (moving) cubic scenes passes its
    self-check — which derives every stored depth again and looks for each span's second record — with direct leaf words
    on and off; the selector never gives such an image a four-wave instance and asks for the kernels with both arms."""
    monkeypatch.setenv("CRT_DIRECT_LEAVES", direct)
    monkeypatch.delenv("CRT_WIDE", raising=False)
    s = SCENES[name]().build(crt)
    chk = s.image_check()
    assert chk["direct_leaves"] == int(direct)
    if direct == "1":
        assert chk["leaf_words_direct_index"] > 0, chk
    else:
        assert chk["leaf_words_direct_index"] == 0 and chk["leaf_words_direct_instance"] == 0, chk
    if name == "instanced":
        assert chk["moving_instances"] == 1 and chk["instances"] == 4, chk
    for want in (-1, 0, -2, -3, -4):
        sel = s.engine_select(want)
        assert sel["wide"] == 0 and sel["direct"] == int(direct), (want, sel)
        assert sel["cold"] & 32 and sel["cold"] & 16 and sel["cold"] & 2, sel  # the cubic bit and what it implies
        assert sel["ext_cold"] == 55 and sel["path_cold"] == 55, sel
    for want in (1, 2):
        with pytest.raises(crt.CrtError) as ei:
            s.engine_select(want)
        assert ei.value.code == -5  # CRT_ERR_UNSUPPORTED
    for wide in ("1", "2"):  # the A/B request falls back
        monkeypatch.setenv("CRT_WIDE", wide)
        for want in (-2, -3):
            assert s.engine_select(want)["wide"] == 0


def test_scenes_without_spans_select_as_before(crt, monkeypatch):
    monkeypatch.delenv("CRT_WIDE", raising=False)
    monkeypatch.delenv("CRT_DIRECT_LEAVES", raising=False)
    sel = cr.scene_tuft().build(crt).engine_select(-1)  # round segments only: the instances it had
    assert sel["cold"] == 16 | 2 and sel["ext_cold"] == 23 and sel["path_cold"] == 23 and sel["wide"] == 0, sel
    b = crt.SceneBuilder()
    b.attach_triangles(*cr.FLOOR)
    b.attach_sphere((0, 1, 0), 0.5)
    sel = b.commit().engine_select(-1)
    assert sel["cold"] & 48 == 0 and sel["ext_cold"] & 48 == 0 and sel["path_cold"] & 48 == 0 and sel["wide"] == 1, sel


# ---------------------------------------------------------------- the USD reader
class _Prim:
    path = "/P"

    def __init__(self, **a):
        self.attrs = a

    def attr(self, n, d=None):
        return self.attrs.get(n, d)


def _basis_f64(basis, cp, t):
    """The basis curve of four control points at parameters t, float64 (the matrices of usd_import.rs:1914-1931)."""
    M = {"bezier": [[-1, 3, -3, 1], [3, -6, 3, 0], [-3, 3, 0, 0], [1, 0, 0, 0]],
         "bspline": [[-1 / 6, 3 / 6, -3 / 6, 1 / 6], [3 / 6, -6 / 6, 3 / 6, 0], [-3 / 6, 0, 3 / 6, 0], [1 / 6, 4 / 6, 1 / 6, 0]],
         "catmullRom": [[-0.5, 1.5, -1.5, 0.5], [1, -2.5, 2, -0.5], [-0.5, 0, 0.5, 0], [0, 1, 0, 0]]}[basis]
    T = np.stack([t ** 3, t ** 2, t, np.ones_like(t)], 1)
    return T @ np.asarray(M, np.float64) @ np.asarray(cp, np.float64)


def test_cubic_basis_curves_become_bezier_spans(crt):
    """_cubic_curve_spans: span counts per basis (vstep 3 / 1 / 1), the converted Bezier curve equal to the basis curve at
    nine parameters within 1e-5 (float64 evaluation of both), bezier the identity bit for bit."""
    spans_of = crt.usda._cubic_curve_spans
    t = np.linspace(0, 1, 9)
    # coordinates with few mantissa bits: the conversion's products and quotients by 3 are then exact, and the identity
    # on a bezier curve is an identity of bits (on arbitrary floats it holds to an ulp or two, as in the reference)
    p7 = np.array([(0, 0, 0), (0.5, 1, 0), (1.5, 1, 0.25), (2, 0, 0.5), (2.5, -1, 0.75), (3.5, -1, 1), (4, 0, 1.25)], np.float32)
    bz = spans_of(_Prim(points=p7, curveVertexCounts=[7], widths=[0.2]))
    assert bz.shape == (2, 14) and bz.dtype == np.float32
    assert np.array_equal(bz[0, 0:12].view(np.uint32), p7[0:4].reshape(-1).view(np.uint32))
    assert np.array_equal(bz[1, 0:12].view(np.uint32), p7[3:7].reshape(-1).view(np.uint32))
    assert spans_of(_Prim(points=p7, curveVertexCounts=[7], basis="bezier", type="cubic")).shape == (2, 14)
    rng = np.random.default_rng(8)
    p5 = rng.uniform(-2, 2, (5, 3)).astype(np.float32)
    for basis in ("bspline", "catmullRom"):
        sp = spans_of(_Prim(points=p5, curveVertexCounts=[5], basis=basis, widths=[0.2]))
        assert sp.shape == (2, 14), basis
        for k in range(2):
            want = _basis_f64(basis, p5[k:k + 4], t)
            got = _basis_f64("bezier", sp[k, 0:12].reshape(4, 3), t)
            assert np.abs(got - want).max() < 1e-5, (basis, k, np.abs(got - want).max())
    # consecutive spans of a bspline / catmullRom curve join: C0 at least
    sp = spans_of(_Prim(points=p5, curveVertexCounts=[5], basis="catmullRom"))
    assert np.abs(sp[0, 9:12] - sp[1, 0:3]).max() < 1e-5 and np.array_equal(sp[1, 0:3], p5[2])  # passes through the points


def test_span_counts_and_width_rules(crt):
    spans_of = crt.usda._cubic_curve_spans
    pts = np.arange(33, dtype=np.float32).reshape(11, 3)
    assert spans_of(_Prim(points=pts, curveVertexCounts=[4])).shape == (1, 14)          # (4 - 4) / 3 + 1
    assert spans_of(_Prim(points=pts, curveVertexCounts=[6])).shape == (1, 14)          # (6 - 4) / 3 + 1: two points left over
    assert spans_of(_Prim(points=pts, curveVertexCounts=[10])).shape == (3, 14)
    assert spans_of(_Prim(points=pts, curveVertexCounts=[10], basis="bspline")).shape == (7, 14)
    assert spans_of(_Prim(points=pts, curveVertexCounts=[3, 4, 2])).shape == (1, 14)    # curves of fewer than four points are skipped
    assert spans_of(_Prim(points=pts, curveVertexCounts=[3, 3])) is None
    assert spans_of(_Prim(points=pts, curveVertexCounts=[4, 9])).shape == (1, 14)        # the second count overruns: the prim stops there
    assert spans_of(_Prim(points=pts, curveVertexCounts=[12])) is None
    assert spans_of(_Prim(points=pts)) is None and spans_of(_Prim(curveVertexCounts=[4])) is None
    assert spans_of(_Prim(points=pts, curveVertexCounts=[4], basis="hermite")) is None
    # radii: 0.5 * max(width, 1e-6) at the span's first and fourth control point; interpolation from the array's length
    w11 = (np.arange(11) + 1).astype(np.float32) * f32(0.01)
    v = spans_of(_Prim(points=pts, curveVertexCounts=[7, 4], widths=w11))  # per vertex
    assert v[:, 12].tolist() == [f32(0.5) * w11[0], f32(0.5) * w11[3], f32(0.5) * w11[7]]
    assert v[:, 13].tolist() == [f32(0.5) * w11[3], f32(0.5) * w11[6], f32(0.5) * w11[10]]
    c = spans_of(_Prim(points=pts, curveVertexCounts=[7, 4], widths=[0.4, 0.2]))  # per curve
    assert c[:, 12].tolist() == [f32(0.2), f32(0.2), f32(0.1)] and c[:, 13].tolist() == c[:, 12].tolist()
    first = spans_of(_Prim(points=pts, curveVertexCounts=[7, 4], widths=[0.4, 0.2, 0.1]))  # neither: the first value
    assert set(first[:, 12].tolist()) == {f32(0.2)}
    assert set(spans_of(_Prim(points=pts, curveVertexCounts=[7, 4]))[:, 13].tolist()) == {f32(0.5)}  # no widths: 1.0
    assert set(spans_of(_Prim(points=pts, curveVertexCounts=[4], widths=[0.0]))[:, 12].tolist()) == {f32(0.5) * f32(1e-6)}


def test_cubic_prims_of_the_stage_are_decoded_on_request(crt, tmp_path):
    import gpu_cubic_cases as gq
    desc, warned = gq.usd_stage(crt, tmp_path, cubic_curves=True)
    names = [g["name"] for g in desc.geoms]
    assert names.count("Tuft") == 1 and "Flattened" not in names  # ONE instance for the cubic prim
    assert not [w for w in warned if "cubic" in w], warned
    tuft = {g["name"]: g for g in desc.geoms}["Tuft"]
    assert tuft["kind"] == "instance"
    proto = desc.protos[tuft["proto"]]
    assert set(proto) == {"spans"} and proto["spans"].shape == (2, 14) and proto["spans"].dtype == np.float32
    assert np.all(proto["spans"][:, 12:14] == f32(0.5) * f32(0.09))
    assert np.array_equal(tuft["l2w"], np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32))
    # the linear prims come out as without the switch
    plain, _ = gq.usd_stage(crt, tmp_path, cubic_curves=False)
    assert [g["name"] for g in plain.geoms] == [n for n in names if n != "Tuft"]
    for a in plain.geoms:
        b = {g["name"]: g for g in desc.geoms}[a["name"]]
        if a["kind"] == "instance":
            assert np.array_equal(plain.protos[a["proto"]]["segments"], desc.protos[b["proto"]]["segments"])
    # default: named and skipped
    default, warned = gq.gc.usd_stage(crt, tmp_path)
    assert "Tuft" not in [g["name"] for g in default.geoms] and len([w for w in warned if "Tuft" in w and "cubic" in w]) == 1
    # and the world builds: the spans' prototype, its instance, its material slot
    scene, mats, _protos = crt.usda.build_world(desc, crt, crt.default_material)
    assert len(mats) == len(desc.geoms) == scene.geometry_count()
    bd = scene.unique_primitive_breakdown()
    assert bd["cubic_curve_spans"] == 2 and bd["curve_segments"] == 7 and bd["instances"] == 3, bd
    scene.image_check()
    sel = scene.engine_select(-3)
    assert sel["wide"] == 0 and sel["cold"] & 32 and sel["path_cold"] == 55, sel
    assert gq.ref_of_desc(desc).n_spans() == 2 and gq.ref_of_desc(desc).n_segments() == 7


# ---------------------------------------------------------------- the brute-force query's own condition
@pytest.mark.parametrize("name", ["one", "tuft", "mixed", "instanced", "deep"])
def test_undecided_rays_stay_under_the_cap(oracle, name):
    """Condition on the seeds of tests/test_gpu_cubic_curves.py: at most 1 % of a test's rays are undecided (a runner-up
    within 8 ulp of the winner), for every t range the GPU tests run; the scenes are what their names say."""
    import gpu_cubic_cases as gq
    if name == "one":
        assert cu.span_depths(gq.scene(name).geoms[1][1])[0] >= 2
    if name == "tuft":
        d = np.concatenate([cu.span_depths(g[1]) for g in gq.scene(name).geoms if g[0] == "cubic"])
        sp = np.concatenate([g[1] for g in gq.scene(name).geoms if g[0] == "cubic"])
        assert len(d) == 64 and set(range(5)) <= set(d.tolist()) and np.all(sp[:, 12] != sp[:, 13]), np.bincount(d)
    if name == "deep":
        assert cu.span_depths(gq.scene(name).geoms[0][1]).tolist() == [10]
    for k, (lo, hi) in enumerate(cu.T_RANGES):
        ref = gq.reference(oracle, name, k)
        und = float((~ref["decided"]).mean())
        print(name, (lo, hi), "undecided %.4f, hit %.3f, occluded %.3f" % (und, ref["hit"].mean(), ref["occluded"].mean()))
        assert und <= cu.UNDECIDED_CAP, (name, lo, hi, und)
        if hi == INF:
            assert ref["hit"].mean() > 0.2  # the rays do meet the scene


def test_undecided_rays_of_the_imported_stage_stay_under_the_cap(crt, oracle, tmp_path):
    import gpu_cubic_cases as gq
    desc, _ = gq.usd_stage(crt, tmp_path)
    ref_scene = gq.ref_of_desc(desc)
    ref = ref_scene.query(oracle, gq.usd_rays(ref_scene), 0.001, INF)
    und = float((~ref["decided"]).mean())
    tuft = [g["name"] for g in desc.geoms].index("Tuft")
    on_spans = int((ref["hit"] & (ref["geom"] == tuft)).sum())
    print("usd: undecided %.4f (%d of %d), on the cubic prim %d" % (und, int((~ref["decided"]).sum()), len(ref["decided"]), on_spans))
    assert und <= cu.UNDECIDED_CAP, und
    assert on_spans > 30
