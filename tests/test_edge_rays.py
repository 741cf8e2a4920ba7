"""The edge corpus (tests/edge_rays.py) on the CPU: the oracle against the exact rational reference (tests/exact_rt.py),
floors on how often the corpus drives the scalar f64 fallback of the packet test (the oracle's coverage counters), known
answers the reference fixes (inclusive range, the later of two exactly coincident triangles wins, the normal_ok
rejection), and the device source of setup_ray / tri_scalar (kernels/traverse.hip.h) compiled as host C++ against both.
The GPU side of the same corpus is tests/test_gpu_edge_rays.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edge_rays as er
import exact_rt as ex
import ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _oracle_answers(scene, cs):
    """Per case: (hit, t, (geom, prim), occluded) from the oracle's batched queries, one launch per range."""
    out = [None] * len(cs)
    for (lo, hi), ix in er.groups(cs).items():
        r = er.rays8([cs[i] for i in ix])
        hf, ids, _front = scene.intersect_n(r, lo, hi)
        occ = scene.occluded_n(r, lo, hi)
        for j, i in enumerate(ix):
            out[i] = (bool(ids[j, 0] != ora.INVALID_ID), float(hf[j, 0]), (int(ids[j, 0]), int(ids[j, 1])), bool(occ[j]))
    return out


def _exact_cases(name):
    """The finite rays of a scene that the exact reference covers (it has no spheres)."""
    return [c for c in er.cases(name) if er.finite(c) and "/sphere/" not in c.label]


@pytest.mark.parametrize("name", er.NAMES)
def test_oracle_agrees_with_the_exact_reference(name):
    """Watertight, no false hit, t within the derived bound, closest (tests/exact_rt.py) for every finite ray."""
    scene, _keep = er.build(ora, name)
    cs = _exact_cases(name)
    tris = {t: er.world_triangles(name, t) for t in (0.0, 1.0)}
    bad = []
    for c, (hit, t, key, occ) in zip(cs, _oracle_answers(scene, cs)):
        for b in ex.check(c, tris[float(c.time)], hit, t, key, occ):
            bad.append((c.label, b))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("name", ["grid", "closed", "instances", "degenerate"])
def test_corpus_drives_the_f64_fallback(name):
    """Packet lanes with an exactly-zero f32 edge function go to the scalar test (triangle.rs:110-172, bvh.rs:551-561 /
    :636-643). The corpus must keep sending lanes there and having them ACCEPTED, for closest and for any hit: floors
    well under what it does today, so that a corpus that quietly stopped exercising the path fails here."""
    floors = {"grid": (2000, 1000, 600, 500), "closed": (4000, 1000, 2000, 500), "instances": (4000, 1000, 3000, 500),
              "degenerate": (30, 8, 20, 6)}[name]
    scene, _keep = er.build(ora, name)
    cs = er.cases(name)
    closest, anyhit = ora.TravStats(), ora.TravStats()
    ora.lib().ora_set_trav_stats(C.byref(closest))
    ora.lib().ora_set_trav_stats_any(C.byref(anyhit))
    try:
        _oracle_answers(scene, cs)
    finally:
        ora.lib().ora_set_trav_stats(None)
        ora.lib().ora_set_trav_stats_any(None)
    got = (closest.fallback_lanes, closest.fallback_accepts, anyhit.fallback_lanes, anyhit.fallback_accepts)
    assert all(g >= f for g, f in zip(got, floors)), (name, got, floors)
    assert closest.fallback_accepts <= closest.fallback_lanes and closest.fallback_accepts <= closest.accepted_hits


def _by_label(name):
    scene, keep = er.build(ora, name)
    cs = er.cases(name)
    return {c.label: (c, a) for c, a in zip(cs, _oracle_answers(scene, cs))}, (scene, keep)


def test_range_bounds_are_inclusive():
    """triangle.rs:160-166: t_s >= t_min det and t_s <= t_max det. Rays with an exact t of 5: t_max = 5, t_min = 5 and
    t_min == t_max == 5 report the hit, one ulp inside too; one ulp outside, or t_max < t_min, does not."""
    res, _k = _by_label("grid")
    up, dn = float(np.nextafter(f32(5), f32(6))), float(np.nextafter(f32(5), f32(4)))
    expect = {(er.T_MIN, 5.0): True, (er.T_MIN, dn): False, (er.T_MIN, up): True, (5.0, er.INF): True,
              (dn, er.INF): True, (up, er.INF): False, (5.0, 5.0): True, (dn, up): True, (6.0, 4.0): False,
              (up, dn): False}
    n = 0
    for label, (c, (hit, t, _key, occ)) in res.items():
        if label.startswith("range/") and "on-plane" not in label:
            want = expect[(c.t_min, c.t_max)]
            assert hit == want and occ == want, (label, hit, occ, want)
            if hit:
                assert t == 5.0, (label, t)
            n += 1
        if "on-plane" in label:  # origin on the plane, t_min = 0: the hit at t = 0
            assert hit and t == 0.0 and occ, label
    assert n == 120


def test_exactly_coincident_triangles_the_later_lane_wins():
    """bvh.rs:533-550: a packet lane replaces the closest hit unless it is FARTHER (`t > closest` skips), so of two
    exactly coincident triangles the later lane wins — through the packet test (interior points) and through the f64
    fallback (points on an edge) alike; across geometries, the later geometry."""
    res, _k = _by_label("degenerate")
    seen = 0
    for label, (c, (hit, _t, key, occ)) in res.items():
        if label.startswith("degen/coincident/"):
            k = int(label.split("/")[2])
            assert hit and occ, label
            assert key == ((2, 1) if k < 3 else (4, 0)), (label, key)
            seen += 1
    assert seen == 15


def test_sliver_with_a_zero_normal_is_skipped_by_closest_hit_only():
    """prim.rs:81-83: a triangle whose f32 normal is exactly zero is never a closest hit (the plate behind it is), but it
    occludes (hit_any does not look at normals, bvh.rs:636-643). At its vertices and on its edge the f32 edge functions
    are exactly 0: the fallback's accepting branch decides both."""
    res, _k = _by_label("degenerate")
    for k in (0, 1, 2):  # the sliver's vertices and a point of its long edge: on it
        for j in (0, 1):
            c, (hit, t, key, occ) = res["degen/sliver/%d/%d" % (k, j)]
            assert occ, c.label
            assert hit and key != (5, 0), (c.label, key, t)  # what lies behind it, never the sliver


# ---------------------------------------------------------------- the device source, compiled as host C++
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("trav_host") / "libtrav_host.so"
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + os.path.join(ROOT, "crust-render_amd", "csrc", "kernels"),
           os.path.join(ROOT, "tests", "host_shade", "trav_host.cpp"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    L = C.CDLL(str(out))
    fp = C.POINTER(C.c_float)
    L.trav_setup_ray.argtypes = [fp, fp, fp, C.POINTER(C.c_int)]
    L.trav_triangle_intersect.argtypes = [fp, fp, fp, C.c_float, C.c_float, fp]
    L.trav_triangle_intersect.restype = C.c_int
    return L


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_setup_ray_of_the_device_source(host):
    """safe_inv3 (bvh.rs:662-668) and the Woop permutation and shear (triangle.rs:41-80) on every corpus direction:
    +-0, below 1e-20, subnormal, ties in |d|, negative dominant axes, unnormalised lengths."""
    n = 0
    for name in er.NAMES:
        for c in er.cases(name):
            if not er.finite(c):
                continue
            o, d = np.ascontiguousarray(c.o, f32), np.ascontiguousarray(c.d, f32)
            out, k = np.zeros(6, f32), (C.c_int * 3)()
            host.trav_setup_ray(_p(o), _p(d), _p(out), k)
            kx, ky, kz = ex.shear_axes([float(x) for x in d])
            assert tuple(k) == (kx, ky, kz), (c.label, tuple(k), (kx, ky, kz))
            with np.errstate(all="ignore"):
                inv = [np.copysign(f32(1e20), x) if abs(x) < f32(1e-20) else f32(1) / x for x in d]
                want = np.array(inv + [d[kx] / d[kz], d[ky] / d[kz], f32(1) / d[kz]], f32)
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (c.label, out, want)
            n += 1
    assert n > 4000


@pytest.mark.parametrize("name", er.NAMES)
def test_tri_scalar_of_the_device_source_against_oracle_and_exact(host, name):
    """Per ray and nearby triangle: the kernels' scalar test (setup_ray + tri_scalar) bit for bit equal to the oracle's
    (triangle.rs:97-106), and both equal to the exact decision wherever it is decided (tests/exact_rt.py: exact shear ->
    edge signs exact -> hit iff every barycentric >= 0; exact range products -> inclusive range), or within the derived
    bounds elsewhere."""
    cs = _exact_cases(name)
    tris = {t: er.world_triangles(name, t) for t in (0.0, 1.0)}
    bad, decided, decided_hits = [], 0, 0
    for c in cs:
        tr = tris[float(c.time)]
        o, d = np.ascontiguousarray(c.o, f32), np.ascontiguousarray(c.d, f32)
        r = ora.ray(o, d)
        for i in ex.candidates(c.o, c.d, [t[3] for t in tr]):
            v = np.ascontiguousarray(np.array(tr[i][3], f32).reshape(9))
            got, want = np.zeros(3, f32), np.zeros(3, f32)
            h_dev = host.trav_triangle_intersect(_p(o), _p(d), _p(v), c.t_min, c.t_max, _p(got))
            h_ora = ora.lib().ora_triangle_intersect(C.byref(r), _p(v[0:3].copy()), _p(v[3:6].copy()), _p(v[6:9].copy()),
                                                     C.c_float(c.t_min), C.c_float(c.t_max), _p(want))
            if h_dev != h_ora or (h_dev and not np.array_equal(got.view(np.uint32), want.view(np.uint32))):
                bad.append((c.label, int(i), "device source != oracle", h_dev, h_ora, got, want))
                continue
            ev = ex.evaluate(c.o, c.d, tr[i][3], c.t_min, c.t_max)
            if ev.decided and not ev.parallel:
                decided += 1
                inside = min(ev.lam()) >= 0
                if ev.range_decided:
                    exact = inside and ev.in_range(c.t_min, c.t_max, 0)
                    if bool(h_ora) != exact:
                        bad.append((c.label, int(i), "decided", h_ora, exact))
                    decided_hits += exact
                elif inside is False and h_ora:
                    bad.append((c.label, int(i), "decided miss accepted"))
            elif h_ora and not ev.possible(c.t_min, c.t_max):
                bad.append((c.label, int(i), "outside the bounds"))
            if h_ora and ev.tol_t != ex.INF and abs(ex.fr(want[0]) - ev.t) > ev.tol_t:
                bad.append((c.label, int(i), "t", float(want[0]), float(ev.t)))
    assert not bad, (len(bad), bad[:4])
    floor = {"grid": (2000, 100), "closed": (4000, 0), "instances": (3000, 0), "degenerate": (40, 0)}[name]
    assert decided >= floor[0] and decided_hits >= floor[1], (decided, decided_hits)  # the exact decisions do get made
