"""Cubic curve spans through the HIP traversal kernels and the renderer: the batched queries, their _stats forms and the
single-ray entry points on every engine instance the selector can give a cubic image, against the brute-force query of
tests/cubic_ref.py (bit for bit on the decided rays, occluded on all of them); the USD stage with its cubic prim decoded;
the renderer's pipelines against each other and against the reference's integrator running on crt_intersect1 /
crt_occluded1. The CPU side — the truth itself, the seeds' condition — is tests/test_cubic_curves.py."""
import copy

import numpy as np
import pytest

import cubic_ref as cu
import curve_ref as cr
import gpu_cubic_cases as gq

pytestmark = pytest.mark.gpu

# engine instance -> (environment, expected crt_scene_engine_select fields): the table of tests/test_gpu_curves.py — the
# three-wave instances; no four-wave instance carries the curve arms, CRT_WIDE=2 on such an image falls back
ENGINES = {
    "flat6": ({"CRT_WIDE": "0", "CRT_POOL_STACK_RT": "6", "CRT_DIRECT_LEAVES": "0"}, {"wide": 0, "direct": 0, "lds_stack": 6}),
    "deep10": ({"CRT_WIDE": "0", "CRT_POOL_STACK_RT": "10", "CRT_DIRECT_LEAVES": "0"}, {"wide": 0, "direct": 0, "lds_stack": 10}),
    "direct": ({"CRT_WIDE": "2", "CRT_DIRECT_LEAVES": "1"}, {"wide": 0, "direct": 1}),
}

_accepted = {}  # (scene, t range) -> {engine: accepted_hits of the closest-hit _stats form}


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", list(gq.SCENES))
def test_queries_match_the_brute_force_reference(crt, oracle, monkeypatch, engine, name):
    import torch
    env, want = ENGINES[engine]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = gq.scene(name).build(crt)
    sel = scene.engine_select(-2)
    assert all(sel[k] == v for k, v in want.items()) and sel["cold"] & 32 and sel["cold"] & 16, (engine, sel)
    scene.image_check()
    rays = gq.rays(name)
    d_rays = crt.rays_to_device(rays)
    n = len(rays)
    for k, (lo, hi) in enumerate(cu.T_RANGES):
        ref = gq.reference(oracle, name, k)
        what = (engine, name, lo, hi)
        hits = crt.hits_to_host(scene.intersect_n(d_rays, lo, hi))
        occ = scene.occluded_n(d_rays, lo, hi).cpu().numpy()
        st_c, st_a = crt.CrtTravStats(), crt.CrtTravStats()
        hits_s = crt.hits_to_host(scene.intersect_n(d_rays, lo, hi, stats=st_c))
        occ_s = scene.occluded_n(d_rays, lo, hi, stats=st_a).cpu().numpy()
        torch.cuda.synchronize()
        cr.compare(ref, hits, occ, what)
        # the _stats forms answer as the plain forms, and count what they answered
        assert np.array_equal(hits_s.view(np.uint8), hits.view(np.uint8)) and np.array_equal(occ_s, occ), what
        n_hit = int((hits["geom_id"] != cu.INVALID).sum())
        assert int(st_c.rays) == n and int(st_a.rays) == n and st_c.queries[0] == n and st_a.queries[0] == n, what
        assert st_c.queries[1] == st_c.instance_descents and st_a.queries[1] == st_a.instance_descents, what
        # accepted closest-hit updates: the round-curve test bounds them by the hits; here also equal on every engine
        # instance (the visiting order is the tree's, not the engine's)
        assert int(st_c.accepted_hits) >= n_hit and int(st_c.accepted_hits) > 0, (what, n_hit, int(st_c.accepted_hits))
        seen = _accepted.setdefault((name, k), {})
        seen[engine] = int(st_c.accepted_hits)
        assert len(set(seen.values())) == 1, (what, seen)
        if name != "instanced":
            assert st_c.instance_descents == 0 and st_c.nodes[1] == 0 and st_c.prims[1] == 0, what
        else:
            assert st_c.instance_descents > 0 and st_c.prims[1] > 0, what
        assert sum(st_c.prims) > 0 and sum(st_a.prims) > 0, what
        floor = 0 if name != "deep" else -1
        curve_wins = int((ref["hit"] & (ref["geom"] != floor)).sum())
        print(what, "hits %d (curves %d), occluded %d, undecided %d, accepted %d" % (n_hit, curve_wins, int(occ.sum()),
                                                                                    int((~ref["decided"]).sum()), int(st_c.accepted_hits)))
        assert curve_wins > n // 10 or hi != float("inf"), (what, curve_wins)
    scene.traversal_error()  # no launch on this scene overflowed a stack


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", list(gq.SCENES))
def test_single_ray_entry_points(crt, oracle, monkeypatch, engine, name):
    """crt_intersect1 / crt_occluded1 on 64 of the rays (the edge list's among them), on every engine instance and
    every t range of the batched test."""
    env, want = ENGINES[engine]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = gq.scene(name).build(crt)
    sel = scene.engine_select(-2)
    assert all(sel[k] == v for k, v in want.items()) and sel["cold"] & 32, (engine, sel)
    rays = gq.rays(name)
    n_seeded = gq.SCENES[name][1]
    n_edge = len(rays) - n_seeded
    assert 0 < n_edge < 64
    pick = np.concatenate([np.arange(0, n_seeded, n_seeded // (64 - n_edge))[:64 - n_edge], np.arange(n_seeded, len(rays))])
    assert len(pick) == 64
    single = [crt.Ray(rays[i, 0:3], rays[i, 3:6], float(rays[i, 6]), int(rays[i, 7:8].view(np.uint32)[0])) for i in pick]
    for k, (lo, hi) in enumerate(cu.T_RANGES):
        ref = gq.reference(oracle, name, k)
        hits = np.zeros(len(pick), crt.HIT_DTYPE)
        hits["geom_id"] = hits["prim_id"] = cu.INVALID
        occ = np.zeros(len(pick), np.uint32)
        for j, r in enumerate(single):
            h = scene.intersect(r, lo, hi)
            if h is not None:
                hits[j] = (h.t, tuple(h.normal), h.front_face, h.u, h.v, h.geom_id, h.prim_id, 0)
            occ[j] = scene.occluded(r, lo, hi)
        sub = {key: v[pick] for key, v in ref.items()}
        dec = sub["decided"]
        z = sub["hit"][dec]
        what = (engine, name, lo, hi)
        assert np.array_equal(hits["geom_id"][dec], sub["geom"][dec]) and np.array_equal(hits["prim_id"][dec], sub["prim"][dec]), what
        assert np.array_equal((hits["t"][dec] * z).view(np.uint32), (sub["t"][dec] * z).view(np.uint32)), what
        assert np.array_equal((hits["normal"][dec] * z[:, None]).view(np.uint32), (sub["normal"][dec] * z[:, None]).view(np.uint32)), what
        assert np.array_equal(hits["front_face"][dec] * z, sub["front"][dec].astype(np.uint32)), what
        assert np.array_equal((hits["u"][dec] * z).view(np.uint32), (sub["u"][dec] * z).view(np.uint32)), what
        assert np.array_equal((hits["v"][dec] * z).view(np.uint32), (sub["v"][dec] * z).view(np.uint32)), what
        assert np.array_equal(occ.astype(bool), sub["occluded"]), what
    scene.traversal_error()


def test_imported_usd_curves_answer_as_the_reference(crt, oracle, tmp_path):
    """The stage of tests/gpu_curve_cases.py through the USD reader with cubic_curves=True: queries on the imported scene
    — linear prims as round segments, the cubic one as two spans — against the truth built from the description."""
    import torch
    desc, warned = gq.usd_stage(crt, tmp_path)
    assert not [w for w in warned if "cubic" in w], warned
    scene, _mats, _protos = crt.usda.build_world(desc, crt, crt.default_material)
    assert scene.engine_select(-2)["cold"] & 32
    ref_scene = gq.ref_of_desc(desc)
    rays = gq.usd_rays(ref_scene)
    ref = ref_scene.query(oracle, rays, 0.001, float("inf"))
    d_rays = crt.rays_to_device(rays)
    hits = crt.hits_to_host(scene.intersect_n(d_rays, 0.001, float("inf")))
    occ = scene.occluded_n(d_rays, 0.001, float("inf")).cpu().numpy()
    torch.cuda.synchronize()
    cr.compare(ref, hits, occ, "usd")
    tuft = [g["name"] for g in desc.geoms].index("Tuft")
    assert int((ref["hit"] & (ref["geom"] == tuft)).sum()) > 30  # the spans are met
    scene.traversal_error()


# ---------------------------------------------------------------- render
def _render_desc(crt):
    """The tuft scene (three span geometries by ray mask over the floor) plus a RectLight, 48 x 32, depth 4."""
    ref = cu.scene_tuft()
    d = crt.usda.SceneDesc()
    tints = [(0.8, 0.8, 0.8), (0.7, 0.3, 0.2), (0.2, 0.6, 0.3), (0.3, 0.3, 0.8)]
    for g, tint in zip(ref.geoms, tints):
        if g[0] == "tris":
            d.geoms.append(dict(kind="mesh", verts=g[1], idx=g[2], mask=g[3], material={"base_color": tint}, name="floor"))
        else:
            d.geoms.append(dict(kind="cubic_curves", spans=g[1], mask=g[2], material={"base_color": tint}, name="tuft"))
    origin, eu, ev = np.array([-1.5, 4, -1.5], np.float32), np.array([0, 0, 3], np.float32), np.array([3, 0, 0], np.float32)
    verts = np.stack([origin, origin + eu, origin + eu + ev, origin + ev]).astype(np.float32)
    rad = (8.0, 8.0, 8.0)
    d.geoms.append(dict(kind="mesh", verts=verts, idx=np.array([(0, 1, 2), (0, 2, 3)], np.uint32), mask=cu.MASK_ALL,
                        material={"_preset": "emissive", "emission_color": rad}, name="light"))
    d.lights.append(dict(kind="rect", geom_id=len(d.geoms) - 1, radiance=np.array(rad, np.float32), origin=origin, edge_u=eu,
                         edge_v=ev, normal=np.array([0, -1, 0], np.float32)))
    d.camera = dict(lookfrom=np.array([0, 2.2, 6.5], np.float32), lookat=np.array([0, 0.5, 0], np.float32),
                    vup=np.array([0, 1, 0], np.float32), vfov_deg=np.float32(40), aspect=np.float32(48 / 32),
                    aperture=np.float32(0), focus_dist=np.float32(6))
    d.settings.update(width=48, height=32, max_depth=4, spp=8)
    return d


def _render(crt, desc, monkeypatch, env, spp=8):
    import torch
    for k in ("CRT_FUSED", "CRT_STAGE_MIN_PATHS", "CRT_LANES", "CRT_LANE_MIN_PATHS", "CRT_WIDE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene, mats, _protos = crt.usda.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], s["max_depth"], s["frame"], s["strategy"], s["filter"],
                                  s["filter_radius"], 0.0)
    r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
    r.render_samples(0, spp)
    torch.cuda.synchronize()
    img, st, pipe, lanes = r.image(), r.stats().as_dict(), r.pipeline(), r.lanes()
    scene.traversal_error()
    return img, st, pipe, lanes


def test_render_pipelines_agree_on_a_cubic_scene(crt, monkeypatch):
    """The fused kernel, the per-stage launches, two lanes and a second run: identical image bits and RayStats counters;
    no pipeline runs a four-wave traversal kernel on the cubic image."""
    desc = _render_desc(crt)
    img, st, pipe, _ = _render(crt, desc, monkeypatch, {"CRT_FUSED": "1"})
    assert pipe["fused"] and not pipe["wide"], pipe
    assert np.isfinite(img).all() and st["camera_rays"] == 48 * 32 * 8 and st["shadow_rays"] > 0 and st["closest_hit"] > st["camera_rays"]
    assert len(np.unique(img.view(np.uint32))) > 500  # a picture, not a constant
    variants = (("per-stage", {"CRT_FUSED": "0", "CRT_STAGE_MIN_PATHS": "1"}, False, 1),
                ("per-stage, asked for four waves", {"CRT_FUSED": "0", "CRT_STAGE_MIN_PATHS": "1", "CRT_WIDE": "1"}, False, 1),
                ("two lanes", {"CRT_LANES": "2", "CRT_LANE_MIN_PATHS": "1"}, None, 2),
                ("second run", {"CRT_FUSED": "1"}, True, 1))
    for tag, env, fused, lanes in variants:
        img2, st2, pipe2, lanes2 = _render(crt, desc, monkeypatch, env)
        assert not pipe2["wide"] and (fused is None or pipe2["fused"] == fused) and lanes2 == lanes, (tag, pipe2, lanes2)
        assert st2 == st, (tag, st2, st)
        assert np.array_equal(img2.view(np.uint32), img.view(np.uint32)), (tag, int((img2.view(np.uint32) != img.view(np.uint32)).sum()))


class _CurvesAsEmpty:
    """usda-module stand-in for ora_world.OracleRenderer: the oracle cannot build curves, and with the seam hooks set it
    never asks its own scene — curve geometries become empty slots, ids unchanged."""

    def __init__(self, usda):
        self.usda = usda

    def build_world(self, desc, api, new_material):
        d = copy.copy(desc)
        d.geoms = [dict(g, kind="empty") if g["kind"] in ("curves", "cubic_curves") else g for g in desc.geoms]
        return self.usda.build_world(d, api, new_material)


def test_reference_integrator_on_the_device_kernel_seam(crt, oracle, monkeypatch):
    """The oracle's trace_path with every intersect / occluded sent to crt_intersect1 / crt_occluded1 on the cubic scene
    (tests/seam_integrator.py; shading stays the oracle's): image bits and counters equal crt_render_samples's — the
    wavefront path on spans against an integrator that is not under test."""
    import ora
    import ora_world
    import seam_cases as sc
    import seam_integrator as si
    desc = _render_desc(crt)
    img, st, _pipe, _ = _render(crt, desc, monkeypatch, {})
    scene, _mats, _protos = crt.usda.build_world(desc, crt, crt.default_material)
    o = ora_world.OracleRenderer(desc, _CurvesAsEmpty(crt.usda))
    host = si.SeamHost(si.DeviceKernel(crt, scene), si.DriversShade(sc.oracle_drivers(), o))
    oimg, ost = host.render(o, 8, 1)
    assert host.calls["intersect"] == ost.closest_hit and host.calls["occluded"] == ost.shadow_rays and ost.shadow_rays > 0
    for f, _t in ora.RayStats._fields_:
        assert getattr(ost, f) == st[f], (f, getattr(ost, f), st[f])
    bad = np.argwhere(oimg.view(np.uint32) != img.view(np.uint32))
    assert bad.shape[0] == 0, (bad.shape[0], bad[:3])
